/*
 * psm_hip.h -- C ABI of the MI355X-native path-tracing core (libpsm_hip.so).
 *
 * This is the drop-in boundary for the hot path of EngineWorld/prismarine-core: the three
 * shader directories ShadersSDK/{radix,hlbvh,raytracing} and the host orchestration in
 * Include/Prismarine/{Radix.hpp,TriangleHierarchy.inl,Pipeline.inl}.  Where the reference passes
 * buffers by SSBO binding number and launches by glDispatchCompute, this ABI passes plain
 * pointers / handles and sizes.  Every entry point names the reference interface it replaces.
 *
 * Conventions
 *   - every function returns 0 on success, a negative psm_status otherwise; nothing throws
 *   - one psm_ctx per GPU, one in-order HIP stream per context (the reference's single GL
 *     context + barrier after every dispatch, Utils.hpp:167-171); all calls are asynchronous
 *     on that stream unless the doc says "synchronises"
 *   - matrices are row-major float[16] / double[16]:  (M v)[i] = sum_j M[4*i+j] v[j]
 *   - "device pointer" = hipMalloc'ed memory on the context's device
 *   - there is NO CPU fallback: without a gfx950 device psm_ctx_create fails
 */
#ifndef PSM_HIP_H
#define PSM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PSM_OK = 0,
    PSM_ERR_INVALID = -1,     /* bad argument / handle */
    PSM_ERR_HIP = -2,         /* a HIP runtime call failed; see psm_last_error */
    PSM_ERR_NO_DEVICE = -3,   /* no gfx950 device visible */
    PSM_ERR_CAPACITY = -4,    /* exceeds an allocated capacity */
    PSM_ERR_STATE = -5,       /* call order violated (e.g. traverse before build) */
    PSM_ERR_PEER = -6         /* tile-sharded frames: another rank reported a failure or did not arrive; every rank
                                 of the communicator returns from the same psm_dist_* call with an error */
} psm_status;

typedef struct psm_ctx psm_ctx;
typedef struct psm_bvh psm_bvh;
typedef struct psm_rt psm_rt;

/* ---------------------------------------------------------------------------------------------
 * context + buffers: replaces the GL utility shim, Include/Prismarine/Utils.hpp:140-178
 * (allocateBuffer<T>, glNamedBufferSubData, glGetNamedBufferSubData, dispatch)
 * ------------------------------------------------------------------------------------------- */
int psm_ctx_create(int device, psm_ctx** out);
/* same, but every launch goes to an existing HIP stream (e.g. the one a framework's collectives run on,
 * so kernels and RCCL calls are ordered without host synchronisation); the stream is not owned */
int psm_ctx_create_on_stream(int device, void* hip_stream, psm_ctx** out);
int psm_ctx_destroy(psm_ctx* ctx);
int psm_ctx_sync(psm_ctx* ctx);
/* measured HBM ceiling of the box: device-to-device copy of `bytes`, best of `reps`, in GB/s of traffic (read + write) */
int psm_ctx_copy_bandwidth(psm_ctx* ctx, size_t bytes, int reps, double* gb_per_s);                 /* synchronises (glFinish, Viewer.cpp:314) */
void* psm_ctx_stream(psm_ctx* ctx);             /* the hipStream_t every launch goes to */
const char* psm_last_error(psm_ctx* ctx);
int psm_device_count(void);

/* handle = the GLuint buffer name the header layer passes around (Utils.hpp:140-150) */
int psm_buf_alloc(psm_ctx* ctx, size_t bytes, uint32_t* handle);
int psm_buf_free(psm_ctx* ctx, uint32_t handle);
int psm_buf_upload(psm_ctx* ctx, uint32_t handle, size_t offset, const void* src, size_t bytes);
int psm_buf_download(psm_ctx* ctx, uint32_t handle, size_t offset, void* dst, size_t bytes); /* synchronises */
int psm_buf_ptr(psm_ctx* ctx, uint32_t handle, void** dev_ptr, size_t* bytes);

/* ---------------------------------------------------------------------------------------------
 * psm::RadixSort::sort, Include/Prismarine/Radix.hpp:47-74 (+ radix/{histogram,pfx-work,
 * permute}.comp): stable ascending sort of (u64 key, u32 value) pairs, result in place.
 * The reference caps n at 2 Mi (Radix.hpp:34-35); here n is bounded by memory only.
 * ------------------------------------------------------------------------------------------- */
int psm_sort_u64_u32(psm_ctx* ctx, uint32_t keys_handle, uint32_t vals_handle, uint32_t n);
int psm_sort_u64_u32_dev(psm_ctx* ctx, uint64_t* d_keys, uint32_t* d_vals, size_t n);
/* Which implementation the sort (and the hierarchy build's sort stage) runs. Results are identical.
 * 2 (default) = hybrid: the LSD passes of the TOP sixteen key bits first (histogram / scan / scatter kernels, two passes),
 * then every workgroup sorts a chunk of whole sixteen-bit bins by the remaining digits in LDS and writes it back once
 * (radix_local): 3 moves of a key through HBM and 7 launches where the reference makes 8 x 3 dispatches (Radix.hpp:57-73).
 * A bin too long for a chunk's LDS is sorted through global memory by one workgroup alone, apart from the small bins before it
 * (slow; correct under every order in which the workgroups run, because a store never shows a neighbour a key of another bin),
 * and the context then falls back to algorithm 0 for good (psm_sort_get_algorithm shows it; setting the algorithm again clears it).
 * 0 = per pass a histogram, a scan (pfx-work.comp:34-70 as its own launch) and a scatter kernel: 256 B/key, 24 launches.
 * 1 = ONE histogram sweep over the keys for all eight digits (histogram.comp:80-116 once instead of per pass) + one
 * scatter launch per pass that finds its tile's bases by decoupled look-back: 200 B/key, 10 launches -- measured slower
 * than 0 on MI355X at every size, kept selectable and under the same parity tests. A look-back spin that
 * times out is reported as PSM_ERR_STATE by the next synchronising call on the context (psm_ctx_sync,
 * psm_buf_download, psm_bvh_get_info, psm_bvh_download): the sort never hangs silently. */
int psm_sort_set_algorithm(psm_ctx* ctx, int algorithm);
/* the algorithm asked for and the one the next sort will run (they differ after a hybrid sort overflowed); either may be NULL */
int psm_sort_get_algorithm(psm_ctx* ctx, int* asked, int* effective);

/* ---------------------------------------------------------------------------------------------
 * psm::TriangleHierarchy, Include/Prismarine/TriangleHierarchy.{hpp,inl}
 * ------------------------------------------------------------------------------------------- */
/* allocate(count), TriangleHierarchy.inl:77-112 (capacity = 2*count there; here exactly max_tris).
 * max_tris <= 2^27 (PSM_ERR_CAPACITY beyond; the reference stops at ~4.19 M, TriangleHierarchy.inl:80). */
int psm_bvh_create(psm_ctx* ctx, size_t max_tris, psm_bvh** out);
int psm_bvh_destroy(psm_bvh* bvh);
/* clearTribuffer(), TriangleHierarchy.inl:161-166 */
int psm_bvh_clear(psm_bvh* bvh);
/* loadMesh(), TriangleHierarchy.inl:173-192 + vertex/loader.comp:32-152 reduced to its result:
 * appends n world-space triangles. positions: 9 floats/triangle; normals: 9 floats/triangle as
 * stored in the normal mosaic (may be NULL -> face normals, loader.comp:119-128); mats: per
 * triangle material id (NULL -> material_id for all). Host pointers. */
int psm_bvh_load_triangles(psm_bvh* bvh, const float* positions, const float* normals,
                           const int32_t* mats, size_t n, int32_t material_id);
/* per-vertex texture coordinates (texcoords mosaic, loader.comp:131): 6 floats per triangle (u,v of the
 * three vertices) for triangles [first, first+n); host pointer. Triangles never given any read as (0,0). */
int psm_bvh_set_texcoords(psm_bvh* bvh, size_t first, const float* uv, size_t n);
/* loadMesh() proper: the accessor / buffer-view virtualisation of
 * Include/Prismarine/VertexInstance.{hpp,inl} + ShadersSDK/vertex/loader.comp:32-152 as one HIP gather
 * kernel: de-index (32- or packed 16-bit indices), read by accessor, transform, normal fallback to the
 * face normal, quads -> two triangles; appended at the current triangle count. */
typedef struct {
    int32_t offset4;      /* VirtualAccessor.offset4 (in floats) */
    int32_t components;   /* VirtualAccessor.components: 0..3 = 1..4 floats (structs.glsl:245-254) */
    int32_t buffer_view;  /* VirtualAccessor.bufferView */
} psm_accessor;
typedef struct {
    int32_t offset4, stride4;  /* VirtualBufferView (structs.glsl:229-232); stride4 <= 0 -> components+1 */
} psm_buffer_view;
typedef struct {
    const float* d_vertices;       /* device pointer: the float pool every accessor indexes (binding 1) */
    size_t vertex_floats;
    const uint32_t* d_indices;     /* device pointer or NULL (binding 2); 16-bit indices packed two per word */
    size_t index_words;
    const psm_accessor* accessors; /* host arrays, copied */
    uint32_t accessor_count;
    const psm_buffer_view* views;
    uint32_t view_count;
    int32_t vertex_accessor, normal_accessor, texcoord_accessor, modifier_accessor; /* -1 = absent */
    float transform[16];           /* row-major t (setTransform, VertexInstance.inl:54-58) */
    float transform_inv[16];       /* row-major inverse(t) */
    int32_t material_id, is_indexed, index16, node_count, primitive_type /* 1 = quads */, loading_offset;
} psm_mesh_desc;
int psm_bvh_load_mesh(psm_bvh* bvh, const psm_mesh_desc* mesh);

/* build(optimization), TriangleHierarchy.inl:206-329: bounds -> fit transform -> Morton+leaves
 * -> radix sort -> emit -> boxes. opt may be NULL (identity). No host synchronisation. */
int psm_bvh_build(psm_bvh* bvh, const double* opt);
/* The reference rebuilds with ~100 dispatches and host polls per frame (TriangleHierarchy.inl:206-329); here a rebuild is
 * 34 launches (C3), and from the second build of a triangle count on they are replayed as ONE captured hipGraph (the host's share of a
 * tiled frame drops from 31 % to 8 % of the wall time). Results are identical; enable = 0 keeps plain launches (default: 1).
 * Per-stage timing (psm_stats_enable) always uses plain launches. */
int psm_bvh_set_build_graph(psm_bvh* bvh, int enable);
/* Refit only (SURVEY f4 "refit-only dynamic updates"; the reference refits as the last stage of build() only): for a hierarchy
 * that has been built and whose triangles were reloaded since -- the same number, in the same order, moved -- recompute the leaf
 * boxes (aabbmaker.comp:165-194, with the transform of the build) and every node's child boxes bottom-up (refit.comp:21-114).
 * Topology, ranges, triangle ids, sorted keys: the build's. PSM_ERR_STATE without a complete build of the current triangle count. */
int psm_bvh_refit(psm_bvh* bvh);

typedef struct {
    uint32_t triangle_count; /* uploaded triangles (tcounter, TriangleHierarchy.inl:209) */
    uint32_t leaf_count;     /* non-degenerate triangles (aabbCounter, :280) */
    int32_t root;            /* root link: >=0 split-gap id of the root, -1 = no traversable tree */
    float transform[16];     /* geometryUniform.transform as M (row-major, not transposed) */
    float bounds_min[4], bounds_max[4]; /* minmax.comp result after the -+1e-5 pad */
} psm_bvh_info;
int psm_bvh_get_info(psm_bvh* bvh, psm_bvh_info* info); /* synchronises */

/* Stage-level entry points (each = one reference dispatch group); psm_bvh_build runs them in
 * order. Exposed so parity tests can check every stage against the oracle. */
int psm_bvh_stage_bounds(psm_bvh* bvh, const double* opt);  /* minmax.comp + host reduce + fit */
int psm_bvh_stage_morton(psm_bvh* bvh);                     /* aabbmaker.comp */
int psm_bvh_stage_sort(psm_bvh* bvh);                       /* Radix.hpp:47-74 */
int psm_bvh_stage_emit(psm_bvh* bvh);                       /* build-new + child-link + refit */

/* Debug / parity downloads (synchronise). `what` (PAIR_BOX, LINK and RANGE -- the nodes in the reference's terms -- are not
 * written by a build, whose traversal reads its own 32-byte record: the first download after a build produces them from the
 * build's still-resident inputs; PSM_ERR_STATE once the next build has begun): */
enum {
    PSM_BVH_KEYS = 0,      /* uint64[leaf_count]   sorted Morton codes (unsorted before stage_sort) */
    PSM_BVH_INDICES = 1,   /* uint32[leaf_count]   MortonIndices */
    PSM_BVH_LEAF_BOX = 2,  /* uint32[4][leaf_count] leaf record boxes (packHalf2 mn.xy mn.zw mx.xy mx.zw), slot order */
    PSM_BVH_LEAF_TRI = 3,  /* int32[leaf_count]    leaf record triangle ids, slot order */
    PSM_BVH_PAIR_BOX = 4,  /* uint32[8][leaf_count-1] child boxes of internal node (split gap) s: left, right */
    PSM_BVH_LINK = 5,      /* int32[2][leaf_count-1]  child links: >=0 internal gap id, <0 leaf: ~triangle */
    PSM_BVH_RANGE = 6,     /* int32[2][leaf_count-1]  sorted-leaf range [first,last] of internal node s */
    PSM_BVH_SORTED_TRI = 7,/* int32[leaf_count]    triangle id of the k-th sorted leaf */
    PSM_BVH_POSITIONS = 8, /* float[9][triangle_count] world-space triangle soup as loaded */
    PSM_BVH_NORMALS = 9,   /* float[9][triangle_count] per-vertex normals as loaded */
    PSM_BVH_MATERIALS = 10,/* int32[triangle_count] */
    PSM_BVH_TEXCOORDS = 11,/* float[6][triangle_count] u,v per vertex */
    PSM_BVH_NODE32 = 12    /* uint32[8][leaf_count-1] the traversal record of internal node s as the build wrote it: 12 fp16 box
                              coordinates (left mn.xyz mx.xyz, right mn.xyz mx.xyz) + the two child links, which a node writes
                              into its PARENT's record */
};
int psm_bvh_download(psm_bvh* bvh, int what, void* dst, size_t bytes);

/* ---------------------------------------------------------------------------------------------
 * psm::Pipeline, Include/Prismarine/Pipeline.{hpp,inl}
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    float lightVector[4]; /* xyz direction, w distance   (Pipeline.inl:93-98) */
    float lightColor[4];  /* rgb, w radius */
    float lightOffset[4];
    float lightAmbient[4];
} psm_light; /* LightUniformStruct, Structs.hpp:165-170 */

typedef struct {
    float diffuse[4], specular[4], transmission[4], emissive[4];
    float ior, roughness, alpharef, unk0f;
    uint32_t diffusePart, specularPart, bumpPart, emissivePart;
    int32_t flags, alphafunc, binding, bitfield;
    int32_t iModifiers0[4];
} psm_material; /* VirtualMaterial, Structs.hpp:240-262 (128 bytes) */

int psm_rt_create(psm_ctx* ctx, psm_rt** out);
int psm_rt_destroy(psm_rt* rt);
/* resizeBuffers(w,h), Pipeline.inl:174-214: ray grid; ray limit = min(4*w*h, 4096*4096) */
int psm_rt_resize_buffers(psm_rt* rt, uint32_t width, uint32_t height);
/* resize(w,h), Pipeline.inl:138-172: display image (presampled / filtered) */
int psm_rt_resize(psm_rt* rt, uint32_t display_width, uint32_t display_height);
/* tile sharding (new): this context owns ray-grid rows [y0,y1). Default all rows. */
int psm_rt_set_tile(psm_rt* rt, uint32_t y0, uint32_t y1);
/* interleaved sharding: this context owns the global 8-row bands g with g % world == rank (balances
 * sky rows against geometry rows; 1.01 max/mean on the Sponza-class view vs 1.21 for 8 contiguous strips).
 * camera() then touches only the owned texels -- except on rank 0, the rank the tiles are gathered to, which
 * also prepares the jitter positions / flags of all other texels because its sample() reads the whole image. */
int psm_rt_set_tile_interleaved(psm_rt* rt, uint32_t rank, uint32_t world);
/* the same with a weighted dealing: the bands go round in periods of P = weights[0] + ... + weights[world-1] <= 64, rank r
 * owning weights[r] bands of every period, laid out by a smooth weighted round-robin (each step every rank's credit grows
 * by its weight, the largest credit -- lowest rank on ties -- takes the band and pays P) so that a rank's bands are
 * spread evenly over the image. weights NULL = 1 each = psm_rt_set_tile_interleaved. The gathering rank also unpacks,
 * fills and samples the whole image, so it is given fewer bands than the workers (8 GPUs: 2 of every 23 against 3). */
int psm_rt_set_tile_weighted(psm_rt* rt, uint32_t rank, uint32_t world, const uint32_t* weights);
/* lightColor/lightVector/lightOffset/lightAmbient + setLightCount, Pipeline.hpp:103-121 */
int psm_rt_set_lights(psm_rt* rt, const psm_light* lights, uint32_t count);
/* environment: constant colour ... */
int psm_rt_set_sky(psm_rt* rt, const float rgba[4]);
/* ... or setSkybox(), Pipeline.hpp:93 + public/environment.glsl:23-26: an equirect RGBA8 image
 * (host pointer, width*height*4 bytes, row 0 first) sampled with GL_LINEAR / clamp-to-edge as the app's
 * loadCubemap() sets it up (Application.hpp:46-54). NULL restores the constant colour. */
int psm_rt_set_skybox(psm_rt* rt, const uint8_t* rgba8, uint32_t width, uint32_t height);
/* TextureSet (TextureSet.inl:15-35,88-122): slot 1..31 of the sampler table
 * surface.comp indexes with diffusePart / specularPart / bumpPart / emissivePart (slot 0 = none,
 * MAX_TEXTURES = 32, surface.comp:46). RGBA8, GL_LINEAR, GL_REPEAT as TextureSet::loadTexture sets them;
 * host pointer, width*height*4 bytes. rgba8 == NULL frees the slot. */
int psm_rt_set_texture(psm_rt* rt, uint32_t slot, const uint8_t* rgba8, uint32_t width, uint32_t height);
/* MaterialSet::loadToVGA + bindWithContext, MaterialSet.inl:13-23 (host pointer, copied) */
int psm_rt_set_materials(psm_rt* rt, const psm_material* mats, uint32_t count, int32_t load_offset);
/* camera(persp, frontSide), Pipeline.inl:279-296 -> camera.comp. camInv/projInv are the inverse
 * matrices the reference uploads (:283-284); `time` replaces the host rand() (:282). Clears the
 * ray counters (clearRays) and this frame's texel sums. */
int psm_rt_camera(psm_rt* rt, const float cam_inv[16], const float proj_inv[16], uint32_t time);
/* cameraUniform.enable360 (switchMode(), Pipeline.inl:128-132; camera.comp:48-59): primary rays over the whole
 * sphere (equirect image) from the camera position instead of through the projection */
int psm_rt_set_camera_mode(psm_rt* rt, int enable360);
/* raycountCache after reloadQueuedRays, Pipeline.inl:325-359 (the >=32 rule of getRayCount,
 * :459-461, is applied by the header layer). Synchronises. */
int psm_rt_ray_count(psm_rt* rt, int32_t* count);
/* intersection(obj), Pipeline.inl:385-405 -> directTraverse.comp. The first call after the ray queue changed
 * (camera, shade, upload_rays, reset_hits) starts the hit chains; further calls with other hierarchies extend
 * them as the reference's ray.hit hand-over does (multi-BVH; directTraverse.comp:219-249,335-346):
 * the search starts at the distance already found and new hits overwrite the front of the chain. At most 16
 * hierarchies of < 2^27 triangles each per queue; psm_rt_shade() then interpolates each hit from the
 * hierarchy that produced it (its `bvh` argument is used when only one was traversed). */
int psm_rt_traverse(psm_rt* rt, psm_bvh* bvh);
/* Which kernel schedule an intersection() runs as. A tuning knob: hits, chains and counters never depend on it
 * (every schedule performs, per ray, the node steps and triangle tests of directTraverse.comp:333-484 in the
 * same order). A wave64 steps as long as its slowest ray; the schedules differ in how they keep lanes busy:
 *   WHOLE       one launch, 64 consecutive rays per wave, run to completion
 *   PHASED      launch k runs at most caps[k] wave-steps, then the rays still under way hand their state (node,
 *               stack, best hit) to a dense continuation queue and the next launch resumes them packed 64 to a
 *               wave; the last launch runs to completion (psm_rt_set_traverse_phases)
 *   ADAPTIVE    the same hand-over, triggered per wave by __ballot / popcount: a wave hands over as soon as fewer
 *               than min_live of its lanes have work left; resume launches are persistent waves striding over the
 *               continuation queue (psm_rt_set_traverse_adaptive)
 *   AUTO        (default) ADAPTIVE while the Pipeline is one of several frames in flight (psm_lanes_*: the other frames'
 *               kernels fill the tails the extra launches add; +5 % on C3, +9 % on C5's scene), WHOLE for a frame on its own (it is bound
 *               by its longest ray, which extra launches serialise) and for intersections under min_rays rays.
 *               Further hierarchies of a multi-BVH queue always run WHOLE. */
enum { PSM_TRAVERSE_AUTO = 0, PSM_TRAVERSE_WHOLE = 1, PSM_TRAVERSE_PHASED = 2, PSM_TRAVERSE_ADAPTIVE = 3 };
int psm_rt_set_traverse_mode(psm_rt* rt, int mode);
/* PHASED: count caps (1..7) -> count + 1 launches, for intersections over at least min_rays rays; count = 0 selects
 * WHOLE. Selects PSM_TRAVERSE_PHASED. */
int psm_rt_set_traverse_phases(psm_rt* rt, const uint32_t* caps, uint32_t count, uint32_t min_rays);
/* ADAPTIVE parameters (does not change the mode): hand over below min_live live lanes (2..64) but not before
 * min_steps wave-steps; a resume launch that finds at most final_rays rays waiting finishes them; at most
 * max_launches launches (2..15) per intersection; intersections under min_rays rays run WHOLE.
 * Defaults: 12, 8, 65536, 4, 2^19. */
int psm_rt_set_traverse_adaptive(psm_rt* rt, uint32_t min_live, uint32_t min_steps, uint32_t final_rays,
                                 uint32_t max_launches, uint32_t min_rays);
/* The solo gear of every schedule (round 4): a traversal wave that is left with at most solo_max rays (0..4; default 1) --
 * and is not in a launch that hands rays over -- stops stepping them one lane each and walks them one after the other with
 * ALL its lanes on one ray: the ray's state is wave-uniform, so the step's decisions are scalar arithmetic instead of lane
 * masks, a lane evaluates one axis of one child box (the same v_fma_mix_f32 on the same operands; tNear / tFar by quad-permute
 * DPP max / min in the order mathlib.glsl:129-193 combines them), the stack lives in the lanes of one register, a leaf's two
 * triangles are tested side by side. A round's tail consists of such waves (a bounce round's longest ray takes 659-1099
 * steps against a mean of 56) and a frame on its own, a tile's launches and every hand-over round's last launch end with
 * them. Per ray nothing changes: the node steps and triangle tests of directTraverse.comp:333-484 in the same order, hits,
 * chains and counters bit-exact. 0 switches the gear off. */
int psm_rt_set_traverse_solo(psm_rt* rt, uint32_t solo_max);
/* forget the chains of the current queue without changing it (the reference's ray.hit = -1, rayslib.glsl:149) */
int psm_rt_reset_hits(psm_rt* rt);
/* applyMaterials + shade, Pipeline.inl:407-436 -> surface.comp + rayshading.comp, then the
 * queue hand-off of reloadQueuedRays (:325-359). `time` replaces rand() (:426). */
int psm_rt_shade(psm_rt* rt, psm_bvh* bvh, uint32_t time);
/* sample(), Pipeline.inl:251-277 -> sampler.comp, deinterlace.comp, filter.comp */
int psm_rt_sample(psm_rt* rt);
/* sample() fed with the frame another Pipeline of the same ray-grid size rendered (its texel sums and jitter
 * coordinates): folds that frame into rt's accumulating image exactly as rt's own sample() would have.
 * Stream-ordered against both contexts, no host synchronisation. */
int psm_rt_sample_from(psm_rt* rt, psm_rt* src);
/* clearSampler(), Pipeline.inl:314-322 (also zeroes presampled: the GL texture starts undefined) */
int psm_rt_clear_sampler(psm_rt* rt);
/* snapHdr()/snapRawHdr(), Pipeline.inl:439-456: display_w*display_h*4 floats to host. Synchronises. */
int psm_rt_snap(psm_rt* rt, float* rgba, int raw);

/* per-texel frame radiance (sum rgb, deposit count) for the tile gather:
 * copy rows [y0,y1) to / from a device pointer (width*(y1-y0)*4 floats). */
int psm_rt_get_texels_dev(psm_rt* rt, uint32_t y0, uint32_t y1, float* d_dst);
int psm_rt_set_texels_dev(psm_rt* rt, uint32_t y0, uint32_t y1, const float* d_src);
/* the same for any tile shape: pack this context's owned texels (row-major over its owned rows) into a
 * dense device buffer of psm_rt_tile_texels() * 4 floats; unpack the dense buffer of tile (rank, world,
 * interleaved != 0) or rows [rank, world) (interleaved == 0) into the full image on the gathering rank */
int psm_rt_tile_texels(psm_rt* rt, uint32_t* count);
int psm_rt_pack_texels_dev(psm_rt* rt, float* d_dst);
int psm_rt_unpack_texels_dev(psm_rt* rt, int interleaved, uint32_t a, uint32_t b, const float* d_src);
/* the gathering rank's side of the gather in one launch: d_all holds the dense tiles of ranks 0..world-1 of an interleaved
 * sharding back to back, stride_floats apart (a multiple of 4, at least the largest tile: what a gather of equal-sized
 * buffers delivers); every texel skip_rank does not own takes its radiance from its owner's tile */
int psm_rt_unpack_tiles_dev(psm_rt* rt, uint32_t world, uint32_t skip_rank, const float* d_all, size_t stride_floats);
/* ray count hand-off without a host read-back: copy the current count to a device int32 (on the
 * context's stream); tell the library the count the host learned elsewhere (e.g. from an all-gather) */
int psm_rt_ray_count_dev(psm_rt* rt, int32_t* d_dst);
int psm_rt_set_ray_count(psm_rt* rt, int32_t count);

/* Debug / parity downloads of the current ray queue and last traversal result (synchronise). */
typedef struct {
    float origin[3], direct[3], color[3];
    int32_t bitfield, texel;
    uint32_t pkey;
} psm_ray;
typedef struct {
    float u, v, t;
    int32_t tri;
} psm_hit;
int psm_rt_download_rays(psm_rt* rt, psm_ray* dst, uint32_t max_rays, uint32_t* count);
/* hits: max_rays*8 entries (chain of ray i at [8*i, 8*i+counts[i])) */
int psm_rt_download_hits(psm_rt* rt, psm_hit* hits, int32_t* counts, uint32_t max_rays);
/* replace the current ray queue (host pointer) -- lets tests drive traverse with chosen rays. count <= currentRayLimit
 * (PSM_ERR_CAPACITY); every ray's texel must lie inside the ray grid, 0 <= texel < w * h (PSM_ERR_INVALID): shading deposits
 * a ray's radiance into the texel it names */
int psm_rt_upload_rays(psm_rt* rt, const psm_ray* src, uint32_t count);
int psm_rt_download_texels(psm_rt* rt, float* sum_rgba, float* coord_xy, int32_t* flags);

/* ---------------------------------------------------------------------------------------------
 * ray queries against a built hierarchy (new; no reference counterpart): batched closest-hit and any-hit over device arrays,
 * beside the Pipeline's wavefront traversal (psm_rt_traverse keeps directTraverse.comp's semantics). Semantics:
 *   - a ray is {origin, tmin, direct, tmax}; direct is normalised with normalize3 (the pipeline's) and t is the distance along
 *     that unit direction, as the oracle's brute force measures it
 *   - the candidates are the hierarchy's leaves (PSM_BVH_LEAF_TRI: the triangles the build kept), by load-order triangle id
 *   - the triangle test is intersectTriangle's arithmetic (tri_test) without the clamp of |det| at 1e-6: invDev = 1 / det,
 *     det == 0 is a miss, the 1e-5 tolerances on u, v, u + v stay. Where |det| >= 1e-6 the values are tri_test's bit for bit
 *   - a hit counts iff tmin <= t <= tmax as floats (no PZERO / INF = 10000 rule). A miss: NaN in any operand, a non-finite
 *     origin or direction, a zero direction, tmin > tmax
 *   - closest: the smallest t; on bit-equal t the lowest triangle id -- the result does not depend on the traversal order.
 *     psm_hit {u, v, t, tri}; a miss is {0, 0, +inf, -1}
 *   - any: d_hit[i] = 1 iff some candidate is hit inside the window, else 0 (uint8_t, torch.bool-compatible)
 *   - a hierarchy of 0 leaves misses everything; one of 1 leaf tests that leaf
 *   - after psm_bvh_refit the refitted boxes are used; as for every refit this is right only for triangles that moved within
 *     the build's bounds (the fit transform and the fp16 box padding are the build's)
 *   - what is promised against a brute force over the leaves: exact on WELL-POSED hits. A hit (ray, triangle, t) is well-posed
 *     iff the point origin + t direct, mapped by the build's transform (psm_bvh_info.transform), lies at most 2.5e-4 (half the
 *     boxes' padding) outside the triangle's normalised bounding box on every axis. Every hit is, except those of a ray almost
 *     in a triangle's plane, where det is rounding noise and t with it. A ray all of whose accepted hits are well-posed gets the
 *     brute force's answer bit for bit. An ill-posed hit of a grazing ray may be reported or not, but is never invented (a
 *     reported hit is a candidate of the brute force, with its u, v, t), and the closest and the any-hit answer never miss a
 *     well-posed hit: the closest is no later in (t, tri) than the best well-posed one
 * Stream-ordered on the hierarchy's context, no host synchronisation (a query can be captured into a graph, except the first one
 * of a context, which allocates its stack area). The stack is sized to the builder's height bound (63 Morton bits + log2 of the
 * largest run of equal codes): no subtree is ever dropped. Any n; d_rays and d_hits 16-byte aligned (PSM_ERR_INVALID otherwise);
 * n = 0 is a no-op; PSM_ERR_STATE before the first build (as psm_rt_traverse). */
typedef struct {
    float origin[3], tmin;
    float direct[3], tmax;
} psm_query_ray; /* 32 B: two 16-byte loads */
int psm_bvh_intersect_dev(psm_bvh* bvh, const psm_query_ray* d_rays, size_t n, psm_hit* d_hits);
int psm_bvh_occluded_dev(psm_bvh* bvh, const psm_query_ray* d_rays, size_t n, uint8_t* d_hit);

/* point queries against a built hierarchy (new; no reference counterpart): closest point and within-radius over device arrays,
 * on the same leaves, stack, context and checks as the ray queries above. Semantics:
 *   - a query is {p, rmax}; the candidates are the hierarchy's leaves (PSM_BVH_LEAF_TRI) by load-order triangle id, a triangle
 *     read as the build stores it: v0, e1 = v1 - v0, e2 = v2 - v0
 *   - closest point on a triangle: Ericson's region test (vertex, edge and face regions) in terms of v0, e1, e2, one fixed
 *     float32 operation order (query.hip closest_on_tri; tests/point_query_model.py restates it). The result is barycentrics u
 *     (weight of e1) and v (weight of e2); the point is c = (v0 + u e1) + v e2 in every region; d2 = dot3(p - c, p - c),
 *     dist = sqrtf(d2)
 *   - degenerate triangles give a finite result for finite input: an edge region is taken only when its denominator is positive
 *     (a zero-length edge never matches; the other regions decide); the face is taken only when aa bb - ab^2 > 2^-16 aa bb
 *     (aa = e1.e1, ab = e1.e2, bb = e2.e2), otherwise the triangle is a sliver and c is the clamped projection onto its longest
 *     edge; the face's u, v are clamped into the triangle (u in [0, 1], v in [0, 1 - u]). The cost of thin triangles, with s the
 *     sine of the angle at v0 and L the longest edge: a face's dist is off by up to ~8 eps / s^2 L (float32 barycentrics), a
 *     sliver's by up to s L (its width) -- up to ~2^-7 L near s = 2^-8, 1e-6 of the size for well-shaped and for collinear or
 *     zero-area triangles. The result is still exact against the same formula over all leaves
 *   - a candidate counts iff dist <= rmax. closest: the smallest d2, on a bit-equal d2 the lowest triangle id -- the result does
 *     not depend on the traversal order. psm_hit {u, v, t = dist, tri}; a miss is {0, 0, +inf, -1}. (tri, u, v) reproduce c
 *   - within: d_hit[i] = 1 iff some candidate counts, else 0 (uint8_t, torch.bool-compatible)
 *   - a non-finite p, or an rmax that is NaN or negative, misses; rmax = +inf is no limit
 *   - 0 / 1 leaves, refit, stream order, capture, alignment (d_points and d_hits 16-byte aligned), NULL checks, n = 0 and
 *     PSM_ERR_STATE before the first build: as for the ray queries */
typedef struct {
    float p[3], rmax;
} psm_point_query; /* 16 B: one 16-byte load */
int psm_bvh_closest_point_dev(psm_bvh* bvh, const psm_point_query* d_points, size_t n, psm_hit* d_hits);
int psm_bvh_within_dev(psm_bvh* bvh, const psm_point_query* d_points, size_t n, uint8_t* d_hit);

/* hit count, inside / outside and signed distance against a built hierarchy (new; no reference counterpart), on the same leaves,
 * stack, context and checks as the queries above. Semantics:
 *   - count: d_count[i] = the number of candidates (the hierarchy's leaves, PSM_BVH_LEAF_TRI) that ray i hits inside its window:
 *     the triangle test and tmin <= t <= tmax of psm_bvh_occluded_dev, which asks "is there one?" of the same predicate. A ray
 *     that is invalid by the ray queries' rules (NaN, non-finite origin or direction, zero direction, tmin > tmax) counts 0; 0
 *     leaves: 0; 1 leaf: that leaf is tested. A sum of integers: it does not depend on the traversal order. Exact on a ray all of
 *     whose accepted hits are well-posed (the ray queries' rule above); otherwise between the number of well-posed hits and the
 *     number of accepted ones -- an ill-posed hit of a grazing ray may be counted or not, and is never invented. The vote and
 *     the sign below are exact for a point all of whose rays are such rays
 *   - inside: for point p the rays {p, tmin = 0, PSM_INSIDE_DIRECTIONS[k], tmax = +inf}, k = 0 .. samples - 1, are counted as
 *     above (each row normalised with normalize3 like every query ray's direction); a ray votes "inside" iff its count is odd,
 *     and d_inside[i] = 1 iff more than half of the rays vote so, else 0 (uint8_t, torch.bool-compatible). samples must be 1, 3
 *     or 5 (PSM_ERR_INVALID otherwise). rmax of the record is ignored: one packed array serves closest point and inside. A
 *     non-finite p is outside
 *   - why a vote: the triangle test keeps a 1e-5 tolerance on u, v, u + v, so a ray that passes within that of an edge shared by
 *     two triangles is counted by both -- one crossing, two hits, the wrong parity. With one ray that happened on 1 of ~20 000
 *     random points of an icosphere and of a torus; the majority of 3 and of 5 was right on all of them
 *   - what is promised: for a closed, consistently crossing surface the right answer, except where more than half of the rays
 *     graze an edge within 1e-5; for an open surface parity means nothing and the result is merely deterministic. A point on the
 *     surface gets whatever its rays' windows give (its own triangle's t is 0 give or take rounding)
 *   - the directions are not axis-aligned and their component ratios are irrational (the normalised (1, sqrt 2, sqrt 3),
 *     (-sqrt 5, 1, sqrt 2), (sqrt 3, -sqrt 7, 1), (-sqrt 2, -sqrt 3, -sqrt 11), (sqrt 7, 1, -sqrt 5)): points of a regular grid
 *     against a mesh whose vertices sit on that grid do not send rays through vertices and edges
 *   - signed distance: d_hits[i] is bit for bit what psm_bvh_closest_point_dev writes for the same query, except that t (the
 *     distance) has its sign bit set when the point is inside by the rule above with the same samples. A miss (no triangle
 *     within rmax, an invalid query) stays {0, 0, +inf, -1} and casts no rays: with a finite rmax this is the narrow-band
 *     distance field, and the points outside the band cost the closest-point walk only (psm_bvh_inside_dev gives the sign of
 *     far points). A distance of exactly 0 comes back as -0.0f when the vote says inside
 *   - d_count 4-byte aligned; everything else (alignment of the inputs and of d_hits, NULL checks, n = 0, PSM_ERR_STATE before
 *     the first build, stream order, capture, refit, 0 / 1 leaves) as for the queries above */
#define PSM_INSIDE_MAX_SAMPLES 5
#define PSM_INSIDE_DIRECTIONS                                                                                      \
    {                                                                                                              \
        {0.4082483f, 0.57735026f, 0.70710677f}, {-0.7905694f, 0.35355338f, 0.5f},                                  \
        {0.52223295f, -0.797724f, 0.30151135f}, {-0.35355338f, -0.4330127f, -0.8291562f},                          \
        {0.7337994f, 0.2773501f, -0.6201737f}                                                                      \
    } /* float[PSM_INSIDE_MAX_SAMPLES][3]: the initialiser of the table, written here once */
int psm_bvh_count_hits_dev(psm_bvh* bvh, const psm_query_ray* d_rays, size_t n, uint32_t* d_count);
int psm_bvh_inside_dev(psm_bvh* bvh, const psm_point_query* d_points, size_t n, uint32_t samples, uint8_t* d_inside);
int psm_bvh_signed_distance_dev(psm_bvh* bvh, const psm_point_query* d_points, size_t n, uint32_t samples, psm_hit* d_hits);

/* k-best queries against a built hierarchy (new; no reference counterpart): the first k hits of a ray and the k
 * nearest triangles of a point, k fixed by the caller, 1 <= k <= PSM_QUERY_K_MAX. The output is n rows of k psm_hit records
 * (d_hits[i * k + s], slot s of query i) and a count per query; there is no allocation, no overflow and no second pass, and with
 * k >= the ray's hit count the row is the complete list. Flat scenes and instanced lists have none; worlds: below
 * (psm_world_first_hits_dev / psm_world_nearest_dev). Semantics:
 *   - first hits: the candidates, the validity of a ray, the triangle test and the window tmin <= t <= tmax are those of
 *     psm_bvh_intersect_dev / psm_bvh_count_hits_dev, unchanged. With c the number psm_bvh_count_hits_dev gives for the ray,
 *     row i holds the min(k, c) counting candidates that are smallest in the lexicographic order (t, tri), ascending: t compared
 *     as floats (-0 == +0, the id then decides), tri unsigned. Each record is {u, v, t, tri} as psm_bvh_intersect_dev writes it
 *   - nearest: the candidates, the validity of a point, closest_on_tri, d2 and dist = sqrtf(d2) <= rmax are those of
 *     psm_bvh_closest_point_dev, unchanged. Row i holds the min(k, c) counting triangles that are smallest in (d2, tri),
 *     ascending -- the key is d2, not dist: two different d2 may share a sqrtf. Each record is {u, v, dist, tri}
 *   - d_count[i] = min(k, c); the slots from d_count[i] on are the miss record {0, 0, +inf, -1}; an invalid query has count 0
 *     and a row of misses
 *   - what follows: slot 0 is bit for bit the record psm_bvh_intersect_dev / psm_bvh_closest_point_dev writes for the query
 *     (bit-equal t / d2 of several triangles -- coincident triangles, a ray within 1e-5 of a shared edge -- are all listed, in id
 *     order); d_count > 0 iff psm_bvh_occluded_dev / psm_bvh_within_dev say 1; the row for k is the first k slots of the row for
 *     any larger k; nothing depends on the traversal order
 *   - k == 0 or k > PSM_QUERY_K_MAX: PSM_ERR_INVALID, nothing is launched. d_hits 16-byte and d_count 4-byte aligned;
 *     everything else (alignment of the inputs, NULL checks, n = 0, PSM_ERR_STATE before the first build, stream order,
 *     capture, refit, 0 / 1 leaves) as for the queries above */
#define PSM_QUERY_K_MAX 16
int psm_bvh_first_hits_dev(psm_bvh* bvh, const psm_query_ray* d_rays, size_t n, uint32_t k, psm_hit* d_hits, uint32_t* d_count);
int psm_bvh_nearest_dev(psm_bvh* bvh, const psm_point_query* d_points, size_t n, uint32_t k, psm_hit* d_hits, uint32_t* d_count);

/* box queries against a built hierarchy (new; no reference counterpart): whether, how many and which of the
 * hierarchy's triangles overlap an axis-aligned box, on the same leaves, stack, context and checks as the queries above. Flat
 * scenes and instanced lists have none; worlds: below (psm_world_box_*_dev: the box stays in world space). Semantics:
 *   - a box {lo, hi} is valid iff its six numbers are finite and lo[k] <= hi[k] on every axis; a point (lo == hi) is valid. An
 *     invalid box answers 0, 0, or count 0 with a row of -1: never an error, as for invalid rays and points. The pads are not read
 *   - the candidates are the hierarchy's leaves (PSM_BVH_LEAF_TRI) by load-order triangle id, a triangle read as the build
 *     stores it: v0, e1 = v1 - v0, e2 = v2 - v0. A triangle the build dropped stays dropped
 *   - a candidate counts iff box_tri(v0, e1, e2, lo, hi): the 13 separating axes of a triangle and a box, in float32, one fixed
 *     operation order, multiplications, additions and compares only (box.hip box_tri; tests/box_query_model.py restates it),
 *     closed: touching counts -- as float32 decides it: where every operation is exact (coordinates on a lattice) contact counts;
 *     elsewhere contact that is exact in real numbers is found or missed by the rounding of the sums.
 *       L = lo - v0, H = hi - v0 per component; f3 = e2 - e1 per component; dot(a, b) = (a0 b0 + a1 b1) + a2 b2
 *       for an axis a: bmin(a) = the sum over a's components of (a_j >= 0 ? a_j L_j : a_j H_j), bmax(a) the same with L and H
 *         swapped; three terms as (s0 + s1) + s2; a component that is zero by construction is left out of the sums and of dot
 *         (the two other terms only, in component order)
 *       an axis with the triangle's projections P (relative to v0) separates iff !(max P >= bmin && min P <= bmax)
 *       the three unit axes k: P = {0, e1_k, e2_k} against [L_k, H_k] directly, no product
 *       the nine edge axes unit_k x f, f = e1, e2, f3: k = x: (0, -f_z, f_y); k = y: (f_z, 0, -f_x); k = z: (-f_y, f_x, 0);
 *         P = {0, dot(a, e2)} for f = e1, P = {0, dot(a, e1)} for f = e2 and for f = f3
 *       the normal axis n = cross3(e1, e2) (psm_math.h): P = {0}
 *       box_tri holds iff no axis separates. max / min of P are selections (p > 0 ? p : 0, p < 0 ? p : 0). A degenerate triangle
 *       gets a finite, deterministic answer: its zero axes separate nothing
 *   - overlaps: d_hit[i] = 1 iff some candidate counts, else 0 (uint8_t, torch.bool-compatible)
 *   - count: d_count[i] = the number c of candidates that count
 *   - triangles: 1 <= k <= PSM_QUERY_K_MAX; row i of d_tris ([n][k]) holds the min(k, c) LOWEST triangle ids that count,
 *     ascending, then -1; d_count[i] = min(k, c). With k >= c the row is the complete list; the row for k is the first k slots of
 *     the row for any larger k
 *   - nothing depends on the traversal order: a flag, a sum, the lowest ids
 *   - k == 0 or k > PSM_QUERY_K_MAX: PSM_ERR_INVALID, nothing is launched, as for the k-best queries. d_boxes 16-byte, d_count
 *     and d_tris 4-byte aligned; everything else (NULL checks, n = 0, PSM_ERR_STATE before the first build -- "box query before
 *     build" --, PSM_ERR_CAPACITY for a hierarchy deeper than the query stack, stream order, capture, refit, 0 / 1 leaves) as
 *     for the queries above. A refused call launches nothing and leaves the output buffers untouched */
typedef struct {
    float lo[3], pad0;
    float hi[3], pad1;
} psm_box_query; /* 32 B: two 16-byte loads */
int psm_bvh_box_overlaps_dev(psm_bvh* bvh, const psm_box_query* d_boxes, size_t n, uint8_t* d_hit);
int psm_bvh_box_count_dev(psm_bvh* bvh, const psm_box_query* d_boxes, size_t n, uint32_t* d_count);
int psm_bvh_box_triangles_dev(psm_bvh* bvh, const psm_box_query* d_boxes, size_t n, uint32_t k, int32_t* d_tris, uint32_t* d_count);

/* sweep queries against a built hierarchy (new; no reference counterpart): where a sphere that moves along a
 * line first touches the hierarchy's triangles, and on which -- the sphere cast of a collision library -- on the same leaves,
 * stack, context and checks as the queries above. Flat scenes and instanced lists have none; worlds: below
 * (psm_world_sweep_*_dev: the sweep in world space). Semantics:
 *   - a query {origin, radius, direct, tmax}: direct is normalised with normalize3 exactly as a query ray's, t is the distance
 *     along that unit direction d, and the sphere of radius `radius` = r has its centre at c(t) = origin + t d for t in [0, tmax]
 *   - a query is valid iff origin and the normalised direction are finite (a zero direction is not), 0 <= r < +inf and
 *     tmax >= 0 (NaN fails both); tmax = +inf is no limit. An invalid query is a miss, never an error. r = 0 is valid: a ray
 *     test with closed edges and none of the ray queries' 1e-5 tolerance, not promised bit-equal to psm_bvh_intersect_dev
 *   - the candidates are the hierarchy's leaves (PSM_BVH_LEAF_TRI) by load-order triangle id, a triangle read as the build
 *     stores it: v0, e1 = v1 - v0, e2 = v2 - v0
 *   - a candidate's first contact is sweep_tri(v0, e1, e2, o, d, r, tmax): the smallest t >= 0 at which the sphere touches the
 *     triangle, in float32, one fixed operation order, one rounding per operation, nothing fused, division and sqrtf correctly
 *     rounded (psm_sweep_dev.h; tests/sweep_query_model.py writes it once over a float type and is its canonical statement).
 *     dot(a, b) = (a0 b0 + a1 b1) + a2 b2; a + s b and a - s b per component, the product first; rr = r r; dd = dot(d, d).
 *       1. the start: d2 = closest_on_tri(v0, e1, e2, o), the point queries' function bit for bit. If sqrtf(d2) <= r the contact
 *          is t = 0 with the closest point's (u, v): a triangle psm_bvh_within_dev (o, r) counts has t == 0.
 *          Otherwise the smallest valid t of the seven features below, in this order, a later one replacing an earlier
 *          one only when its t is smaller (a tie keeps the earlier: face, v0, v1, v2, edge v0 v1, edge v0 v2, edge v1 v2).
 *          started(t) = t > 0 ? t : 0: a feature the sphere moves towards and already reaches at the start is a contact at
 *          t = 0. In real numbers the start test has then fired; in float32 the start test and the features round
 *          independently, and a sphere that rests on a triangle within rounding of r -- where every sweep leaves it -- and moves
 *          into it is found by one or the other, never by neither. So t == 0 without psm_bvh_within_dev counting the triangle
 *          happens only within rounding of dist(o, triangle) = r, for a sphere that is moving in
 *       2. the face, only under closest_on_tri's sliver rule det = aa bb - ab ab > 2^-16 (aa bb) (aa = dot(e1, e1), ab =
 *          dot(e1, e2), bb = dot(e2, e2)): n = cross3(e1, e2), w0 = o - v0, s0 = dot(n, w0), sd = dot(n, d), rn = r sqrtf(dot(n,
 *          n)); needs s0 sd < 0; t = started(((s0 > 0 ? rn : -rn) - s0) / sd); w = w0 + t d, p1 = dot(w, e1), p2 =
 *          dot(w, e2), u = (bb p1 - ab p2) / det, v = (aa p2 - ab p1) / det; counts iff u >= 0, v >= 0, u + v <= 1 (closed, no
 *          tolerance)
 *       3. the vertices q = v0, v0 + e1, v0 + e2 by closest approach: m = o - q, t0 = -dot(m, d) / dd, l = m + t0 d, qq = rr -
 *          dot(l, l); needs t0 > 0 and qq >= 0; t = started(t0 - sqrtf(qq / dd)); (u, v) = (0, 0), (1, 0), (0, 1)
 *       4. the edges (q, e) = (v0, e1), (v0, e2), (v0 + e1, e2 - e1), the axial part removed first: ee = dot(e, e) > 0, m = o - q,
 *          sm = dot(m, e) / ee, sn = dot(d, e) / ee, mp = m - sm e, dp = d - sn e, a = dot(dp, dp); needs a > 0, t0 = -dot(mp, dp)
 *          / a > 0 and qq = rr - dot(l, l) >= 0 with l = mp + t0 dp; t = started(t0 - sqrtf(qq / a)); counts iff s = sm + t sn lies in
 *          [0, 1]; (u, v) = (s, 0), (0, s), (1 - s, s)
 *       The contact counts iff t <= tmax (closed: a sweep that ends exactly at contact hits). The closest-approach form, not
 *       the textbook quadratic, because the quadratic's constant term cancels in float32 (DESIGN.md 4.17 has the figures).
 *       Degenerate triangles get a finite, deterministic answer: a zero-length edge is skipped and its vertices decide, a
 *       sliver has no face and its edges and vertices decide -- near the sliver threshold the face's barycentric noise
 *       (closest_on_tri) can move a contact by ~2^-7 of the longest edge
 *   - sweep sphere: d_hits[i] = {u, v, t, tri} of the smallest t over all candidates, on a bit-equal t the lowest triangle id:
 *     nothing depends on the traversal order. (u, v) is the contact point on the triangle, (v0 + u e1) + v e2; the contact
 *     normal is (c(t) - contact) / r. A miss is {0, 0, +inf, -1}
 *   - sweep occluded: d_hit[i] = 1 iff some candidate has a contact within [0, tmax], else 0 (uint8_t, torch.bool-compatible):
 *     the predicate isfinite(t) of the first call; the walk ends at the first such candidate
 *   - d_sweeps and d_hits 16-byte aligned; everything else (NULL checks, n = 0, PSM_ERR_STATE before the first build -- "sweep
 *     query before build" --, PSM_ERR_CAPACITY for a hierarchy deeper than the query stack, stream order, capture, refit, 0 / 1
 *     leaves) as for the ray queries. A refused call launches nothing and leaves the output buffers untouched */
typedef struct {
    float origin[3], radius;
    float direct[3], tmax;
} psm_sweep_query; /* 32 B: two 16-byte loads, where a query ray's are */
int psm_bvh_sweep_sphere_dev(psm_bvh* bvh, const psm_sweep_query* d_sweeps, size_t n, psm_hit* d_hits);
int psm_bvh_sweep_occluded_dev(psm_bvh* bvh, const psm_sweep_query* d_sweeps, size_t n, uint8_t* d_hit);

/* triangle queries against a built hierarchy (new; no reference counterpart): whether, how many and which of
 * the hierarchy's triangles meet a given triangle -- the narrow phase of mesh against mesh -- on the same leaves, stack, context
 * and checks as the queries above. A world has them over its posed instances (psm_world_tri_*_dev below); flat scenes and instanced lists have none. Semantics:
 *   - a query {a, b, c} is valid iff its nine numbers are finite; a degenerate query triangle (a segment, a point) is valid. An
 *     invalid query answers 0, 0, or count 0 with a row of -1: never an error, as for invalid rays, points and boxes. The pads
 *     are not read
 *   - the candidates are the hierarchy's leaves (PSM_BVH_LEAF_TRI) by load-order triangle id, a triangle read as the build
 *     stores it: v0, e1 = v1 - v0, e2 = v2 - v0. A triangle the build dropped stays dropped
 *   - a candidate counts iff tri_tri(v0, e1, e2, a, b, c): a separating-axis test in float32, one fixed operation order,
 *     multiplications, additions, subtractions and compares only -- no division, no square root, nothing fused
 *     (psm_tri_dev.h tri_tri; tests/tri_query_model.py restates it) --, closed: touching counts, as float32 decides it: where
 *     every operation is exact (coordinates on a lattice) contact counts; elsewhere contact that is exact in real numbers is
 *     found or missed by the rounding of the sums.
 *       everything is relative to the stored v0: A = a - v0, B = b - v0, C = c - v0 per component, one rounding each; the stored
 *       triangle is {0, e1, e2} with the edges e1, e2, e3 = e2 - e1; the query's edges are g1 = B - A, g2 = C - A, g3 = C - B
 *       dot(x, y) = (x0 y0 + x1 y1) + x2 y2; cross(x, y) = cross3 (psm_math.h): (x1 y2 - y1 x2, x2 y0 - y2 x0, x0 y1 - y0 x1)
 *       on an axis ax the stored triangle's interval [tmin, tmax] is the min / max of {0, dot(ax, e1), dot(ax, e2)} and the
 *         query's [qmin, qmax] that of {dot(ax, A), dot(ax, B), dot(ax, C)}; min / max of {x, y, z} are selections:
 *         m = y < x ? y : x, then z < m ? z : m (max: with >)
 *       an axis separates iff !(tmax >= qmin && qmax >= tmin): a NaN bound separates
 *       the pair counts iff none of these 20 axes separates, in this order:
 *         1. the three unit axes k, no product: {0, e1_k, e2_k} against {A_k, B_k, C_k} -- box_tri's unit axes for the query's
 *            bounding box [min(a, b, c), max(a, b, c)] (the subtraction is monotonic), which the prune's proof rests on
 *         2. n = cross(e1, e2), then m = cross(g1, g2)
 *         3. the nine cross(e_i, g_j), i outer, j inner
 *         4. cross(n, e_i), i = 1, 2, 3, then cross(m, g_j), j = 1, 2, 3: the in-plane axes that decide coplanar pairs
 *       (2) and (3) are the complete set for two triangles that are not coplanar, (4) the complete 2-D set for coplanar ones, (1)
 *       is redundant in real numbers. A zero axis (a degenerate triangle, parallel edges) projects everything to 0 and separates
 *       nothing: a degenerate triangle on either side gets whatever the remaining axes say, finite and deterministic
 *     magnitudes: the in-plane axes are products of three coordinate differences and are multiplied by a fourth; with d the
 *     largest coordinate difference between any two of the pair's six vertices, every intermediate is below 12 d^4, so nothing
 *     overflows while d < 2^30 (and nothing that decides underflows to 0 while the differences exceed 2^-30). Beyond that an
 *     overflow gives an infinity or a NaN, an axis that holds one separates and the pair is missed; there is no guard
 *   - overlaps: d_hit[i] = 1 iff some candidate counts, else 0 (uint8_t, torch.bool-compatible); the walk ends at the first
 *   - count: d_count[i] = the number c of candidates that count
 *   - triangles: 1 <= k <= PSM_QUERY_K_MAX; row i of d_ids ([n][k]) holds the min(k, c) LOWEST triangle ids that count,
 *     ascending, then -1; d_count[i] = min(k, c). With k >= c the row is the complete list; the row for k is the first k slots of
 *     the row for any larger k
 *   - nothing depends on the traversal order: a flag, a sum, the lowest ids
 *   - not covered: the intersection segment itself, a posed query mesh in one call, k > PSM_QUERY_K_MAX, flat scenes and
 *     instanced lists
 *   - k == 0 or k > PSM_QUERY_K_MAX: PSM_ERR_INVALID, nothing is launched. d_tris 16-byte, d_count and d_ids 4-byte aligned;
 *     everything else (NULL checks, n = 0, PSM_ERR_STATE before the first build -- "triangle query before build" --,
 *     PSM_ERR_CAPACITY for a hierarchy deeper than the query stack, stream order, capture, refit, 0 / 1 leaves) as for the
 *     queries above. A refused call launches nothing and leaves the output buffers untouched */
typedef struct {
    float a[3], pad0;
    float b[3], pad1;
    float c[3], pad2;
} psm_tri_query; /* 48 B: three 16-byte loads */
int psm_bvh_tri_overlaps_dev(psm_bvh* bvh, const psm_tri_query* d_tris, size_t n, uint8_t* d_hit);
int psm_bvh_tri_count_dev(psm_bvh* bvh, const psm_tri_query* d_tris, size_t n, uint32_t* d_count);
int psm_bvh_tri_triangles_dev(psm_bvh* bvh, const psm_tri_query* d_tris, size_t n, uint32_t k, int32_t* d_ids, uint32_t* d_count);

/* clearance queries against a built hierarchy (new; no reference counterpart): how far a given triangle is
 * from the hierarchy's triangles -- which one is nearest, at what distance and at which two points, and whether any is within
 * a radius -- on the same leaves, stack, context and checks as the queries above. The triangle family's counterpart of
 * psm_bvh_closest_point_dev / psm_bvh_within_dev. Flat scenes, instanced lists, worlds and posed meshes have none. Semantics:
 *   - a query {a, rmax, b, c} is valid iff its nine coordinates are finite and rmax is neither NaN nor negative; -0 is 0 and
 *     +inf is no limit (the point queries' rules). A degenerate query triangle (a segment, a point) is valid. An invalid query
 *     is a miss, never an error. The pads are not read
 *   - the candidates are the hierarchy's leaves (PSM_BVH_LEAF_TRI) by load-order triangle id, a triangle read as the build
 *     stores it: v0, e1 = v1 - v0, e2 = v2 - v0
 *   - a candidate's distance is tri_dist(v0, e1, e2, a, b, c) in float32, one fixed operation order, one rounding per
 *     operation, nothing fused, division and sqrtf correctly rounded (psm_tri_dist_dev.h; tests/tri_dist_query_model.py writes
 *     it once over a float type and is its canonical statement).
 *       everything is relative to the stored v0, as tri_tri has it: A = a - v0, B = b - v0, C = c - v0, g1 = B - A, g2 = C - A,
 *       g3 = C - B, e3 = e2 - e1: the overlap test and the distances see the same rounded coordinates
 *       1. fifteen features, in this order, each giving four weights (u, v) of e1, e2 and (s, t) of g1, g2:
 *            F0 - F2   the query's vertices a, b, c against the stored triangle: (u, v) of closest_on_tri(v0, e1, e2, a | b | c),
 *                      the point queries' function bit for bit; (s, t) = (0, 0), (1, 0), (0, 1)
 *            F3 - F5   the stored vertices 0, e1, e2 against the query triangle: (s, t) of closest_on_tri(A, g1, g2, 0 | e1 | e2);
 *                      (u, v) = (0, 0), (1, 0), (0, 1)
 *            F6 - F14  the nine edge pairs e_i, g_j, i outer, j inner (tri_tri's order), by seg_seg(p1, d1, p2, d2) with
 *                      (p1, d1) = (0, e1), (0, e2), (e1, e3) and (p2, d2) = (A, g1), (A, g2), (B, g3); a weight x along
 *                      e1 / e2 / e3 is (u, v) = (x, 0) / (0, x) / (1 - x, x), a weight y along g1 / g2 / g3 likewise for (s, t)
 *          seg_seg: the clamped closest points of two segments (Ericson 5.1.9): r = p1 - p2, a = dot(d1, d1), e = dot(d2, d2),
 *          b = dot(d1, d2), c = dot(d1, r), f = dot(d2, r), den = a e - b b; skew = den > 2^-16 (a e);
 *          x0 = clamp01(skew ? (b f - c e) / den : 0); y = e > 0 ? clamp01((b x0 + f) / e) : 0; x = a > 0 ? clamp01((b y - c) / a) : 0
 *          (a zero-length segment is its point; a pair whose den is within its own rounding -- sin^2 of the angle at most
 *          2^-16, closest_on_tri's sliver threshold -- is parallel; clamp01 takes a NaN to 0: finite weights in [0, 1] for
 *          every finite input)
 *       2. every feature's d2 is computed the same way from its weights: Q = (A + s g1) + t g2, P = u e1 + v e2 per component,
 *          d2 = dot(Q - P, Q - P): (tri, u, v, s, t) reproduce the value exactly. The smallest d2 wins; on a bit-equal d2 the
 *          first in the order (F0 is taken first; a later feature replaces the winner iff its d2 is smaller)
 *       3. if tri_tri(v0, e1, e2, a, b, c) holds (the triangle queries' test above) the pair's d2 is 0: two triangles that meet
 *          have clearance 0, and an edge that pierces a face leaves all fifteen features positive. The weights reported are
 *          STILL step 2's winner: where the two boundaries come closest, not a point of the intersection. tri_tri's 20 axes are
 *          complete for two triangles with an area; where neither has one (a segment against a segment or a point), and for a
 *          segment lying in a triangle's plane, it lacks axes and may hold for a pair that is apart (its block above: "whatever
 *          the remaining axes say"): such a pair is at 0 too -- the side a clearance check errs on, and what
 *          psm_bvh_tri_overlaps_dev answers for it
 *       4. dist = sqrtf(d2); the candidate counts iff dist <= rmax (closed)
 *     accuracy: on well-shaped triangles dist is within 2^-19 L of the real distance, L the largest coordinate difference of the
 *     pair's six vertices relative to v0 (DESIGN.md 4.23 has the measured figure); a sliver on either side keeps
 *     closest_on_tri's per-triangle bound. Coordinate differences beyond 2^30 overflow tri_tri (above), beyond
 *     2^63 the squares: d2 is then +inf or NaN and the candidate does not count
 *   - closest: d_hits[i] = {u, v, dist, tri, s, t, 0, 0} of the smallest d2 over all candidates that count, on a bit-equal d2
 *     the lowest triangle id: nothing depends on the traversal order. The first 16 bytes are a psm_hit. The nearest point of the
 *     stored triangle is (v0 + u e1) + v e2, that of the query triangle (a + s (b - a)) + t (c - a). A miss, or an invalid
 *     query, is {0, 0, +inf, -1, 0, 0, 0, 0}
 *   - within: d_flag[i] = 1 iff some candidate counts, else 0 (uint8_t, torch.bool-compatible): the predicate tri >= 0 of the
 *     first call; the walk ends at the first such candidate
 *   - not covered: a posed mesh in one call and per-pose clearance, flat scenes and instanced lists (a world has them:
 *     "clearance queries over a world" below), the k nearest triangles, penetration depth, an intersection point at dist = 0
 *   - d_queries and d_hits 16-byte aligned; everything else (NULL checks, n = 0, PSM_ERR_STATE before the first build --
 *     "clearance query before build" --, PSM_ERR_CAPACITY for a hierarchy deeper than the query stack, stream order, capture,
 *     refit, 0 / 1 leaves) as for the queries above. A refused call launches nothing and leaves the output buffers untouched */
typedef struct {
    float a[3], rmax;
    float b[3], pad0;
    float c[3], pad1;
} psm_tri_dist_query; /* 48 B: three 16-byte loads; psm_tri_query's layout with rmax where its first pad is */
typedef struct {
    float u, v, dist; /* the first 16 bytes: a psm_hit */
    int32_t tri;
    float s, t, zero0, zero1;
} psm_tri_hit; /* 32 B: two 16-byte stores */
int psm_bvh_tri_closest_dev(psm_bvh* bvh, const psm_tri_dist_query* d_queries, size_t n, psm_tri_hit* d_hits);
int psm_bvh_tri_within_dev(psm_bvh* bvh, const psm_tri_dist_query* d_queries, size_t n, uint8_t* d_flag);

/* mesh queries against a built hierarchy (new; no reference counterpart): the triangle queries above with the
 * query triangles taken from ANOTHER built hierarchy `other` of the same context, at each of p rigid poses, in one call: does
 * part B at this pose cut part A, where, and with which triangles. `bvh` is the hierarchy being queried. Nothing is downloaded,
 * posed on the host or packed: no psm_tri_query record exists anywhere. Flat scenes, instanced lists and worlds have none.
 * Semantics:
 *   - poses: HOST memory, p x 12 floats, each a row-major 3 x 4 [R | T] that takes a point of other's object space into bvh's
 *     (x' = R x + T), read at the call as psm_instance is and checked as its matrix is (finite; R^T R within 1e-5 of the
 *     identity in every entry, in double: rotations and reflections)
 *   - T = other's loaded triangle count (psm_bvh_info.triangle_count). Outputs are indexed by pose q and by other's load-order
 *     triangle id t, like everything else in this header: d_hit [p], d_count [p][T], d_ids [p][T][k]
 *   - the query of (pose m, triangle t of other) comes from other's STORED record (v0, e1 = v1 - v0, e2 = v2 - v0), in float32,
 *     one rounding per operation, nothing fused, with fwd_point / fwd_vec of the world box queries (below):
 *       a = fwd_point(m, v0),  b = a + fwd_vec(m, e1),  c = a + fwd_vec(m, e2)
 *     At the identity pose the query is the stored triangle, not the loaded one: a = v0 and b = fl(v0 + e1) =
 *     fl(v0 + fl(v1 - v0)), which can differ from the loaded vertex v1 by an ulp (and c from v2)
 *   - the answer for (m, t) is BIT FOR BIT what psm_bvh_tri_overlaps_dev / psm_bvh_tri_count_dev / psm_bvh_tri_triangles_dev
 *     answer for psm_tri_query {a, b, c} on bvh: the same tri_tri, the same prune on the same bounding box, the same k rule
 *     (1 <= k <= PSM_QUERY_K_MAX), the same rows (the min(k, c) lowest ids of bvh that count, ascending, then -1; d_count =
 *     min(k, c)). A query whose posed image holds a non-finite number (an overflow) answers as an invalid psm_tri_query: 0, or
 *     count 0 with a row of -1
 *   - a triangle of other that its build dropped (not in PSM_BVH_LEAF_TRI) answers count 0 with a row of -1 at every pose
 *   - overlaps: d_hit[q] = 1 iff some leaf of other at pose q meets some leaf of bvh -- the OR over the pose's queries --, else 0
 *   - other == bvh is allowed: a self-intersection check at the identity. Every leaf then meets at least ITSELF (the query is
 *     the stored triangle: A = 0), and its neighbours that share a vertex or an edge; the caller discounts these
 *   - nothing depends on the traversal order, on either hierarchy's tree or on timing: a flag, sums, the lowest ids. Query i
 *     of the launch is pose i / L and other's leaf i % L by ascending triangle id (L its leaf count): the queries, and their
 *     order, of the triangle queries over the same posed triangles packed in load order (DESIGN.md 4.21 has what other's
 *     Morton order measured: slower)
 *   - refusals, all before any launch and with the outputs untouched: NULL bvh or other (PSM_ERR_INVALID, no message: there is
 *     no context to keep one); then, with a message on bvh's context, NULL poses or outputs, d_count / d_ids not 4-byte aligned,
 *     k == 0 or k > PSM_QUERY_K_MAX (PSM_ERR_INVALID); either hierarchy not built (PSM_ERR_STATE, "mesh query before build");
 *     bvh deeper than the query stack (PSM_ERR_CAPACITY); hierarchies of different contexts (PSM_ERR_INVALID); a pose that is
 *     not finite or not rigid, named by its index (PSM_ERR_INVALID); p x T >= 2^32 (PSM_ERR_CAPACITY)
 *   - p == 0 returns PSM_OK and touches nothing (it is answered before everything but the NULL handles). Otherwise the outputs
 *     are cleared in stream order (0, rows of -1) before the one kernel: other without leaves launches none; bvh without leaves
 *     answers 0 / -1 everywhere
 *   - the poses go to the device as a world's do: copied on the context's stream into a buffer the context owns, and the call
 *     waits for that copy (and, in the same wait, reads other's leaf count). The call therefore synchronises the context's
 *     stream once before its launch and cannot be captured into a graph; the kernel itself is stream-ordered like every query.
 *     That upload, the wait and the clears are what a call costs beside the triangle queries on records that are already
 *     packed and resident (measured: 0.03 to 0.05 ms at 2 304 answers; DESIGN.md 4.21 times them apart from the kernel)
 *   - study knob, no part of the contract: the overlaps kernel lets a lane skip its walk when its pose's flag already reads 1,
 *     by itself only in launches of more than PSM_QUERY_GRID_CAP waves; the environment variable PSM_MESH_SKIP = 0 / 1, read
 *     at each call, forces that off / on (tools/query_bench.py meshes, tests/test_gpu_mesh_query.py). The answer is the same
 *   - not covered: a mesh against a world, a flat scene or an instanced list; a dual-tree walk that prunes whole subtrees of
 *     other; the intersection segments; k > PSM_QUERY_K_MAX
 *     (since added: a mesh against a world -- "mesh queries over a world" below, psm_world_mesh_*_dev) */
int psm_bvh_mesh_overlaps_dev(psm_bvh* bvh, psm_bvh* other, const float* poses, size_t p, uint8_t* d_hit);
int psm_bvh_mesh_count_dev(psm_bvh* bvh, psm_bvh* other, const float* poses, size_t p, uint32_t* d_count);
int psm_bvh_mesh_triangles_dev(psm_bvh* bvh, psm_bvh* other, const float* poses, size_t p, uint32_t k, int32_t* d_ids, uint32_t* d_count);

/* mesh clearance against a built hierarchy (new; no reference counterpart): the clearance queries above with
 * the query triangles taken from ANOTHER built hierarchy `other` of the same context, at each of p rigid poses, in one call,
 * and the ONE nearest pair of each pose: how close part B comes to part A at this pose, and where -- what a placement search, a
 * tolerance check ("at least 2 mm between A and B at each of these 1 000 poses") and a collision margin ask. Unless said
 * otherwise below, everything is as psm_bvh_mesh_count_dev has it: bvh, other, poses, p, T = other's loaded triangle count,
 * indexing by other's load-order triangle id, how the poses are checked and uploaded, the one synchronisation, no graph
 * capture. Semantics:
 *   - rmax / r: one scalar per call. NaN or negative is not a refusal: it answers as psm_bvh_tri_closest_dev does for such a
 *     query, a miss everywhere. -0 is 0, +inf is no limit
 *   - mesh_closest: d_hits [p][T]. The record of (pose q, triangle t of other) is BIT FOR BIT what psm_bvh_tri_closest_dev
 *     writes for psm_tri_dist_query {a, rmax, b, c}, with a, b, c the posed triangle of the mesh queries
 *     (a = fwd_point(m, v0), b = a + fwd_vec(m, e1), c = a + fwd_vec(m, e2)). A triangle that other's build dropped reads
 *     the miss record {0, 0, +inf, -1, 0, 0, 0, 0} at every pose, as does one whose posed image is not finite
 *   - mesh_clearance: d_hits [p], one psm_mesh_hit per pose. Let t* be the lowest t among the triangles of other whose
 *     mesh_closest record has the smallest dist, comparing the float32 dist as stored. The record is that triangle's
 *     mesh_closest record, bit for bit, with other = t*. A pose where no pair counts reads {0, 0, +inf, -1, 0, 0, -1, 0}.
 *     The rule is stated on dist, not on d2, so that it can be checked from the public outputs alone. (u, v) weigh e1, e2 of
 *     bvh's triangle tri; (s, t) weigh b - a, c - a of the posed triangle `other`: the two witness points, both in bvh's space
 *   - mesh_within: d_flag [p]; d_flag[q] = 1 iff mesh_clearance at rmax = r finds a pair at pose q, else 0. The walk of a
 *     triangle ends at its first pair that counts
 *   - nothing depends on the traversal order, on either hierarchy's tree or on timing. Inside the clearance launch the lanes
 *     of a pose share one 64-bit word, (bits(dist) << 32) | t, lowered by atomic minimum and read back as a smaller rmax;
 *     nobody waits on it; every value it takes is the dist of a real pair that counts, so the final word is (the smallest
 *     dist, t*) under every schedule (mesh_dist.hip and DESIGN.md 4.24 have the argument). The weights do not travel through
 *     the word: a second, tiny launch walks triangle t* of each pose again and writes the record
 *   - refusals: the mesh queries' own, with the same texts under these names, all before any launch and with the outputs
 *     untouched: NULL bvh or other (PSM_ERR_INVALID, no message); NULL poses or output; d_hits not 16-byte aligned
 *     (PSM_ERR_INVALID); either hierarchy not built (PSM_ERR_STATE, "mesh query before build"); bvh deeper than the query stack
 *     (PSM_ERR_CAPACITY); hierarchies of different contexts; a pose that is not finite or not rigid, named by its index
 *     (PSM_ERR_INVALID); p x T >= 2^32 (PSM_ERR_CAPACITY). p == 0 returns PSM_OK and touches nothing
 *   - other without leaves launches no walk and answers a miss everywhere; bvh without leaves answers a miss everywhere
 *   - study knobs, no part of the contract, read at each call: PSM_MESH_BOUND = 0 / 1 decides whether the clearance kernel's
 *     lanes read the shared word (0: every lane walks with rmax alone; the answer is the same; the default is 1; 2 and 3 are
 *     the variants DESIGN.md 4.24 compares); PSM_MESH_SKIP = 0 / 1 is the within kernel's skip of a pose whose flag already
 *     reads 1, as psm_bvh_mesh_overlaps_dev has it
 *   - not covered: clearance over an InstanceWorld, a QueryScene or an InstancedScene; a per-pose rmax; the k closest pairs; a
 *     dual-tree walk that prunes whole subtrees of other; penetration depth; graph capture of the call
 *     (since added: clearance over an InstanceWorld -- "mesh clearance over a world" below, psm_world_mesh_closest_dev /
 *     _within_dev / _clearance_dev) */
typedef struct {
    float u, v, dist; /* the first 24 bytes: a psm_tri_hit */
    int32_t tri;
    float s, t;
    int32_t other; /* t*: the triangle of other, -1 on a miss */
    float zero;
} psm_mesh_hit; /* 32 B: two 16-byte stores */
int psm_bvh_mesh_closest_dev(psm_bvh* bvh, psm_bvh* other, const float* poses, size_t p, float rmax, psm_tri_hit* d_hits);
int psm_bvh_mesh_within_dev(psm_bvh* bvh, psm_bvh* other, const float* poses, size_t p, float r, uint8_t* d_flag);
int psm_bvh_mesh_clearance_dev(psm_bvh* bvh, psm_bvh* other, const float* poses, size_t p, float rmax, psm_mesh_hit* d_hits);

/* scene queries: the seven queries above over several hierarchies at once (new; no reference counterpart).
 * A scene is an ordered list of G built hierarchies of ONE context, 1 <= G <= PSM_SCENE_MAX_GEOMETRIES, passed per call (there
 * is no scene handle). The limit is 32 because the per-geometry table then travels with the launch (32 x four pointers = 1 KB
 * of kernel arguments): it needs no device allocation and cannot go stale when a geometry is rebuilt. Semantics:
 *   - the candidates are the leaves of all geometries, each identified by (geom, tri): geom is the index in the list, tri that
 *     hierarchy's load-order triangle id. Every per-candidate rule is the single-hierarchy query's, unchanged: the triangle
 *     test, closest_on_tri, the windows and radii, which queries are invalid, the 1e-5 tolerances. Only the combination across
 *     the geometries is new, and a scene answers exactly as the psm_bvh_* queries of its geometries combined by these rules:
 *   - intersect, closest_point: the smallest t (d2) over the whole scene; on a bit-equal value the lexicographically lowest
 *     (geom, tri). d_hits[i] is the psm_hit the winning hierarchy alone would have written, d_geom[i] its index, -1 on a miss
 *     (d_hits[i] then {0, 0, +inf, -1}). d_geom must be non-NULL and 4-byte aligned. tmax / rmax apply over the whole scene
 *   - occluded, within: the OR over the geometries
 *   - count_hits: the sum over the geometries
 *   - inside: ray k votes "inside" iff its crossings SUMMED OVER ALL GEOMETRIES are odd; then the majority vote of
 *     psm_bvh_inside_dev. A closed surface split over several hierarchies therefore behaves like the unsplit one -- which no
 *     combination of per-hierarchy inside answers can give. Nested or overlapping bodies behave as they do inside one hierarchy:
 *     parity of all crossings (a point in a cavity between two nested shells is outside, whichever geometries hold the shells)
 *   - signed_distance: the scene's closest-point record (and d_geom) with the scene's inside sign; a miss casts no rays
 *   - the same hierarchy may appear more than once: the lower index wins every tie (its count and parity count once per entry)
 *   - a refitted geometry behaves as a refitted hierarchy does; a geometry of 0 leaves contributes nothing
 *   - a geometry is where its triangles are; a rigid transform per entry is what the instanced scene queries below add
 *     (psm_instances_*_dev). There is no top-level hierarchy over the geometries (every geometry is entered by every query,
 *     pruned from its root on) and no more than 32 geometries
 * Checks: geoms == NULL, count == 0 or count > PSM_SCENE_MAX_GEOMETRIES: PSM_ERR_INVALID. Then every entry, the whole call being
 * refused with a message that names the first failing index: a NULL entry or one of another context than the others
 * (PSM_ERR_INVALID), one that is not built (PSM_ERR_STATE), one too deep for the query stack (PSM_ERR_CAPACITY). The list is
 * checked for n == 0 too; after that n == 0 is a no-op. The data pointers, their alignment and samples as for the psm_bvh_* forms.
 * Stream-ordered on the geometries' context, no host synchronisation, one launch per query (signed distance: two); capturable
 * into a graph after the context's first query of any kind; the context's one stack area serves these queries too. */
#define PSM_SCENE_MAX_GEOMETRIES 32
int psm_scene_intersect_dev(psm_bvh* const* geoms, uint32_t count, const psm_query_ray* d_rays, size_t n, psm_hit* d_hits,
                            int32_t* d_geom);
int psm_scene_occluded_dev(psm_bvh* const* geoms, uint32_t count, const psm_query_ray* d_rays, size_t n, uint8_t* d_hit);
int psm_scene_count_hits_dev(psm_bvh* const* geoms, uint32_t count, const psm_query_ray* d_rays, size_t n, uint32_t* d_count);
int psm_scene_closest_point_dev(psm_bvh* const* geoms, uint32_t count, const psm_point_query* d_points, size_t n, psm_hit* d_hits,
                                int32_t* d_geom);
int psm_scene_within_dev(psm_bvh* const* geoms, uint32_t count, const psm_point_query* d_points, size_t n, uint8_t* d_hit);
int psm_scene_inside_dev(psm_bvh* const* geoms, uint32_t count, const psm_point_query* d_points, size_t n, uint32_t samples,
                         uint8_t* d_inside);
int psm_scene_signed_distance_dev(psm_bvh* const* geoms, uint32_t count, const psm_point_query* d_points, size_t n,
                                  uint32_t samples, psm_hit* d_hits, int32_t* d_geom);

/* instanced scene queries: the seven scene queries over an ordered list of INSTANCES, an instance being a built hierarchy and a
 * rigid transform (new; no reference counterpart). A body that moves costs nothing to move: the next call reads
 * the new matrix, and one built hierarchy can stand at up to PSM_SCENE_MAX_GEOMETRIES poses. The list lives in host memory and
 * is read at the call; count is 1 .. PSM_SCENE_MAX_GEOMETRIES; the same bvh may appear many times with different transforms.
 * Semantics:
 *   - instance k answers exactly what psm_bvh_*_dev on its hierarchy answers for the query MOVED INTO ITS OBJECT SPACE, and the
 *     scene combines the instances' answers by the rules of the scene queries above, unchanged: closest hit and closest point
 *     take the smallest value, on a bit-equal value the lowest (inst, tri); occluded and within the OR; count_hits the sum;
 *     inside sums the parity over all instances before the vote; signed_distance is the closest point with the scene's sign,
 *     and a miss casts no rays. tmax and rmax apply over the whole scene
 *   - the canonical move, one fixed float32 operation order (nothing is contracted): with world_from_object = [R | T] and
 *     d = x - T per component, x'_j = (R[0][j] d.x + R[1][j] d.y) + R[2][j] d.z. A direction goes through the same rotation
 *     without the subtraction: a ray's direction is rotated as given, and the single-hierarchy rule then normalises it as it
 *     does today. tmin, tmax and rmax pass through unchanged
 *   - validity is judged per instance on the moved query. A query that is invalid in world space is invalid in every instance
 *     (NaN and infinity propagate through the move)
 *   - inside: the rays {p, 0, PSM_INSIDE_DIRECTIONS[k], +inf} are WORLD rays from p, each moved per instance
 *   - what comes back: psm_hit {u, v, t, tri} holds the OBJECT-SPACE values of the winning instance, d_inst[i] its index in the
 *     list (-1 on a miss, the hit then {0, 0, +inf, -1}). (tri, u, v) reproduce the object-space point (v0 + u e1) + v e2; the
 *     caller maps it to world space with that instance's matrix, world = R * object + T
 *   - reflections (det R = -1) are accepted: distance and parity do not depend on winding. Scale and shear are out of scope and
 *     refused (below). The bound of that check also means that t and dist are world distances only to within 1e-5 relative
 *   - a refitted or rebuilt hierarchy is used as it then is, at every pose it stands at
 * Checks, all on the host and before any device is touched; the call is refused with a message that names the first failing
 * index: insts == NULL, count == 0 or count > PSM_SCENE_MAX_GEOMETRIES: PSM_ERR_INVALID. Then every entry: a NULL bvh or one of
 * another context than the others (PSM_ERR_INVALID); then every matrix, in double: a non-finite entry, or an R whose R^T R
 * differs from the identity by more than 1e-5 in any entry (PSM_ERR_INVALID); then every hierarchy: not built (PSM_ERR_STATE),
 * too deep for the query stack (PSM_ERR_CAPACITY). The list is checked for n == 0 too; after that n == 0 is a no-op. The data
 * pointers, their alignment (d_inst: non-NULL, 4 bytes) and samples as for the psm_scene_* forms.
 * Stream-ordered on the hierarchies' context, no host synchronisation, no device allocation, one launch per query (signed
 * distance: two); capturable into a graph after the context's first query of any kind. The transforms travel in the kernel
 * arguments (32 x (four pointers + 12 floats) = 2560 B): a replayed graph answers with the poses it was CAPTURED with, whatever
 * the host's list holds by then; a plain call always reads the list as it is. */
typedef struct {
    psm_bvh* bvh;
    float world_from_object[12];   /* row-major 3x4 [R | T]: world = R * object + T */
} psm_instance;                    /* host memory, read at the call */
int psm_instances_intersect_dev(const psm_instance* insts, uint32_t count, const psm_query_ray* d_rays, size_t n, psm_hit* d_hits,
                                int32_t* d_inst);
int psm_instances_occluded_dev(const psm_instance* insts, uint32_t count, const psm_query_ray* d_rays, size_t n, uint8_t* d_hit);
int psm_instances_count_hits_dev(const psm_instance* insts, uint32_t count, const psm_query_ray* d_rays, size_t n, uint32_t* d_count);
int psm_instances_closest_point_dev(const psm_instance* insts, uint32_t count, const psm_point_query* d_points, size_t n,
                                    psm_hit* d_hits, int32_t* d_inst);
int psm_instances_within_dev(const psm_instance* insts, uint32_t count, const psm_point_query* d_points, size_t n, uint8_t* d_hit);
int psm_instances_inside_dev(const psm_instance* insts, uint32_t count, const psm_point_query* d_points, size_t n, uint32_t samples,
                             uint8_t* d_inside);
int psm_instances_signed_distance_dev(const psm_instance* insts, uint32_t count, const psm_point_query* d_points, size_t n,
                                      uint32_t samples, psm_hit* d_hits, int32_t* d_inst);

/* instance worlds: the seven queries over a top-level tree of instances (new; no reference counterpart).
 * The instanced queries above enter every instance for every query and end at 32 entries. A world is a handle that owns, on
 * the device, the table of up to PSM_WORLD_MAX_INSTANCES instances and a binary tree over their padded world-space boxes; a
 * query walks the tree and enters only the instances it can reach. Semantics, in one sentence: a world of N instances answers
 * every query exactly as psm_instances_*_dev would over the same ordered list if that list could be N long -- candidates,
 * windows, rmax, validity per instance on the moved query, the float32 move, inside summing each ray's crossings over all
 * instances before the vote, the record (the winning instance's object-space u, v, t, tri; d_inst its index in the list) and
 * ties going to the lexicographically lowest (inst, tri). The tree never shows in an answer: every box is padded and every
 * prune slackened beyond the worst difference between the world-space box test and the object-space candidate test.
 *   - psm_world_create(ctx, capacity): capacity 1 .. PSM_WORLD_MAX_INSTANCES; NULL on failure (psm_last_error says why)
 *   - psm_world_set_instances(world, insts, count): the list checks of the instanced queries with the same messages (a NULL
 *     bvh, another context than the world's, a pose that is non-finite or not rigid -- in double --, a hierarchy that is not
 *     built or too deep), all before any device work; count > capacity: PSM_ERR_CAPACITY; count == 0 empties the world. Then
 *     the table is uploaded, every instance's box is computed on the device from its hierarchy's triangles (nothing is read
 *     back), and the tree is built on the context's stream: Morton keys of the box centres with the instance index as the
 *     tie-break, the library's sort, one emit kernel, one bottom-up box pass. Synchronises once, to read the tree's depth
 *   - depth: a walk uses one stack for both levels. A world whose tree depth plus its deepest hierarchy's depth bound plus one
 *     exceeds the 96 entries of the query stack is refused (PSM_ERR_CAPACITY) and LEFT EMPTY
 *   - psm_world_set_transforms(world, first, count, m12): new poses (12 floats each) for instances first .. first + count - 1,
 *     checked as above; boxes and tree are rebuilt, no hierarchy is
 *   - staleness: the table holds device pointers. Every hierarchy carries a generation that each build bumps (a load or a clear
 *     leaves the hierarchy un-built until its next build or refit); the world records it at psm_world_set_instances, and every
 *     query (and psm_world_set_transforms) looks, once per distinct hierarchy, for a generation that differs or a hierarchy
 *     that is not built: PSM_ERR_STATE with a message naming the first stale instance, and nothing is launched. Set the
 *     instances again. A hierarchy must outlive the worlds that hold it. A REFIT (reload the same count, psm_bvh_refit) does
 *     not bump the generation but moves the triangles out of the boxes: call psm_world_set_transforms over the whole range
 *     (with the poses as they are) after it, and the world is exact again
 *   - an empty world (never set, emptied, or refused for its depth) answers every query with misses; no query kernel runs
 *   - the seven queries: data arguments, their checks and n == 0 as the psm_instances_* forms; stream-ordered on the world's
 *     context, no host synchronisation, one launch (signed distance: two) */
#define PSM_WORLD_MAX_INSTANCES 65536
typedef struct psm_world psm_world;
psm_world* psm_world_create(psm_ctx* ctx, uint32_t capacity);
int psm_world_destroy(psm_world* world);
int psm_world_set_instances(psm_world* world, const psm_instance* insts, uint32_t count);
int psm_world_set_transforms(psm_world* world, uint32_t first, uint32_t count, const float* m12);
uint32_t psm_world_count(const psm_world* world);
int psm_world_intersect_dev(psm_world* world, const psm_query_ray* d_rays, size_t n, psm_hit* d_hits, int32_t* d_inst);
int psm_world_occluded_dev(psm_world* world, const psm_query_ray* d_rays, size_t n, uint8_t* d_hit);
int psm_world_count_hits_dev(psm_world* world, const psm_query_ray* d_rays, size_t n, uint32_t* d_count);
int psm_world_closest_point_dev(psm_world* world, const psm_point_query* d_points, size_t n, psm_hit* d_hits, int32_t* d_inst);
int psm_world_within_dev(psm_world* world, const psm_point_query* d_points, size_t n, uint8_t* d_hit);
int psm_world_inside_dev(psm_world* world, const psm_point_query* d_points, size_t n, uint32_t samples, uint8_t* d_inside);
int psm_world_signed_distance_dev(psm_world* world, const psm_point_query* d_points, size_t n, uint32_t samples, psm_hit* d_hits,
                                  int32_t* d_inst);

/* k-best queries over a world (new; no reference counterpart): a ray's first k hits and a point's k nearest
 * triangles over every instance of the world, in one launch, 1 <= k <= PSM_QUERY_K_MAX. d_hits[i * k + s] and d_inst[i * k + s]
 * are slot s of query i, d_count[i] the number of filled slots. Flat scenes and instanced lists (psm_scene_*, psm_instances_*)
 * have no k-best query: a world over the same ordered list answers as they would. Semantics:
 *   - candidates: exactly those of psm_world_count_hits_dev / psm_world_within_dev. Per instance the query is moved by the
 *     canonical float32 move and its validity is judged on the moved query; a ray candidate passes the triangle test with
 *     tmin <= t <= tmax, a point candidate passes closest_on_tri with sqrtf(d2) <= rmax, d2 the instance's own value for its
 *     own moved point
 *   - rows: with c the world's count of candidates, row i holds the min(k, c) candidates smallest in the lexicographic order
 *     (value, inst, tri), ascending: value is t (resp. d2, not the distance), compared as a float (-0 == +0); inst and tri are
 *     compared unsigned. A record is the winning instance's object-space {u, v, t | dist, tri}, as psm_world_intersect_dev /
 *     psm_world_closest_point_dev write it, and d_inst the instance's index in the list
 *   - d_count[i] = min(k, c); the slots from d_count[i] on hold {0, 0, +inf, -1} and inst = -1; an invalid query has count 0
 *     and a row of misses
 *   - what follows: slot 0 and its inst are bit for bit the record and d_inst of psm_world_intersect_dev /
 *     psm_world_closest_point_dev; the count is min(k, psm_world_count_hits_dev); it is positive iff psm_world_occluded_dev /
 *     psm_world_within_dev say 1; the row for k is a prefix of the row for any larger k; nothing depends on the tree or the
 *     visit order (coincident instances tie on every hit and are listed inst ascending); a world of N instances answers as
 *     the flat instanced list would if it could be N long and had the query
 *   - k == 0 or k > PSM_QUERY_K_MAX: PSM_ERR_INVALID, nothing is launched. d_hits 16-byte, d_inst and d_count 4-byte aligned,
 *     none NULL; the stale check, n == 0, stream order and capture as for the other world queries; an empty world answers
 *     without a query kernel: n x k miss records, inst = -1, counts 0 */
int psm_world_first_hits_dev(psm_world* world, const psm_query_ray* d_rays, size_t n, uint32_t k, psm_hit* d_hits, int32_t* d_inst,
                             uint32_t* d_count);
int psm_world_nearest_dev(psm_world* world, const psm_point_query* d_points, size_t n, uint32_t k, psm_hit* d_hits, int32_t* d_inst,
                          uint32_t* d_count);

/* box queries over a world (new; no reference counterpart): whether, how many and which (instance, triangle)
 * pairs of a world overlap an axis-aligned box given in WORLD space, in one launch. A posed box would be an oriented box in
 * object space; the contract avoids it: the box stays in world space and is never moved, the candidate triangle is posed
 * forward. Flat scenes and instanced lists (psm_scene_*, psm_instances_*) have no box query. Semantics:
 *   - box validity, closedness and the answer for an invalid box are those of the box queries against a built hierarchy:
 *     six finite numbers, lo[k] <= hi[k]; a point is a box; an invalid box answers 0, 0, or count 0 with rows of -1. The box is
 *     not moved, so there is no per-instance validity
 *   - the candidates are the pairs (inst, tri): inst an index of the world's ordered list, tri a leaf of that instance's
 *     hierarchy (PSM_BVH_LEAF_TRI), stored as v0, e1, e2
 *   - with m = world_from_object[12] of the instance, in float32, one rounding per operation, nothing fused (the order
 *     the world's instance boxes are made in):
 *       fwd_point(m, x)_k = ((m[4k] * x.x + m[4k+1] * x.y) + m[4k+2] * x.z) + m[4k+3]
 *       fwd_vec  (m, d)_k =  (m[4k] * d.x + m[4k+1] * d.y) + m[4k+2] * d.z
 *     the candidate counts iff box_tri(fwd_point(m, v0), fwd_vec(m, e1), fwd_vec(m, e2), lo, hi), box_tri the function of the
 *     box queries above, unchanged, bit for bit. The edges are R e1 and R e2 -- not differences of posed vertices
 *   - the flat answer, which a world reproduces exactly, is taken over the ordered instance list and all leaves of every member:
 *       overlaps: d_hit[i] = 1 iff some candidate counts, else 0
 *       count: d_count[i] = the number c of candidates that count, summed over the instances (uint32)
 *       triangles: 1 <= k <= PSM_QUERY_K_MAX; rows i of d_tri and d_inst ([n][k] int32 each) hold the min(k, c) LOWEST pairs
 *         (inst, tri) that count in lexicographic order, ascending (inst and tri compared unsigned); the slots past
 *         d_count[i] = min(k, c) hold -1 in both. The row for k is a prefix of the row for any larger k; coincident instances
 *         list every shared triangle once per instance, the lowest instance first
 *   - nothing depends on the tree, its prune or the order of the walk: a flag, a sum, the lowest pairs
 *   - k == 0 or k > PSM_QUERY_K_MAX: PSM_ERR_INVALID, nothing is launched, as for the k-best queries. d_boxes 16-byte, d_count,
 *     d_tri and d_inst 4-byte aligned, none NULL; the stale check, the depth budget, n == 0, stream order and capture as for the
 *     other world queries; an empty world answers 0 / 0 / count 0 and rows of -1 without a query kernel. A refused call
 *     launches nothing and leaves the output buffers untouched */
int psm_world_box_overlaps_dev(psm_world* world, const psm_box_query* d_boxes, size_t n, uint8_t* d_hit);
int psm_world_box_count_dev(psm_world* world, const psm_box_query* d_boxes, size_t n, uint32_t* d_count);
int psm_world_box_triangles_dev(psm_world* world, const psm_box_query* d_boxes, size_t n, uint32_t k, int32_t* d_tri, int32_t* d_inst,
                                uint32_t* d_count);

/* sweep queries over a world (new; no reference counterpart): where a sphere that moves along a line given in
 * WORLD space first touches a triangle of a posed instance, and whether it touches one, over every instance of a world in one
 * launch. The answer is exactly the brute force over the ordered instance list, whatever the tree looks like. Flat scenes and
 * instanced lists (psm_scene_*, psm_instances_*) have no sweep. Semantics:
 *   - a query is a psm_sweep_query {origin, radius, direct, tmax} in world space, valid under the rule of the sweep queries
 *     against a built hierarchy: origin finite, normalize3(direct) finite (a zero direction is not), 0 <= radius < +inf,
 *     tmax >= 0. An invalid query is a miss, never an error
 *   - per instance with m = world_from_object[12] the query moves as a world ray does: o' = inst_point(m, origin), d' =
 *     normalize3(inst_rotate(m, direct)) -- the origin and the direction as given, not the normalised world direction -- in
 *     float32, one rounding per operation; radius and tmax are unchanged, because a pose is rigid. An instance in which o' or d'
 *     is not finite is skipped
 *   - the candidates are the pairs (inst, tri), tri a leaf of the instance's hierarchy (PSM_BVH_LEAF_TRI); a candidate's first
 *     contact is sweep_tri(v0, e1, e2, o', d', radius) of the sweep queries above, unchanged, bit for bit, and counts iff
 *     t <= tmax (closed)
 *   - sweep sphere: d_hits[i] = the winning instance's object-space {u, v, t, tri} and d_inst[i] its index in the list: the
 *     smallest t over all candidates, on a bit-equal t the lexicographically lowest (inst, tri), compared unsigned: coincident
 *     instances tie to the lowest instance. A miss is {0, 0, +inf, -1} with d_inst[i] = -1. t is the distance the centre
 *     travels along d' in the instance, equal to the world distance to 1.5e-5 (the pose check); the world contact point is the
 *     pose of (v0 + u e1) + v e2
 *   - sweep occluded: d_hit[i] = 1 iff some candidate counts, else 0: the predicate isfinite(t) of the first call
 *   - carried over: the start test of a candidate is closest_on_tri on the moved origin, the function and the moved point of
 *     psm_world_within_dev bit for bit, so a pair psm_world_within_dev(origin, radius) counts has t == 0
 *   - nothing depends on the tree, its prune or the order of the walk
 *   - d_sweeps and d_hits 16-byte, d_inst 4-byte aligned, none NULL; the stale check, the depth budget, n == 0, stream order
 *     and capture as for the other world queries; an empty world answers misses / 0 without a query kernel. A refused call
 *     launches nothing and leaves the output buffers untouched */
int psm_world_sweep_sphere_dev(psm_world* world, const psm_sweep_query* d_sweeps, size_t n, psm_hit* d_hits, int32_t* d_inst);
int psm_world_sweep_occluded_dev(psm_world* world, const psm_sweep_query* d_sweeps, size_t n, uint8_t* d_hit);

/* triangle queries over a world (new; no reference counterpart): whether, how many and which (instance,
 * triangle) pairs of a world meet a triangle given in WORLD space, in one launch: the narrow phase of a mesh against the posed
 * bodies of a world. The contract is the box queries' over a world with the candidate test of the triangle queries against a
 * built hierarchy. Flat scenes and instanced lists (psm_scene_*, psm_instances_*) have no triangle query. Semantics:
 *   - a query is a psm_tri_query {a, b, c} in world space and is never moved. It is valid iff its nine numbers are finite; a
 *     segment or a point is a valid query; an invalid query answers 0, 0, or count 0 with rows of -1. The query is not moved,
 *     so there is no per-instance validity
 *   - the candidates are the pairs (inst, tri): inst an index of the world's ordered list, tri a leaf of that instance's
 *     hierarchy (PSM_BVH_LEAF_TRI), stored as v0, e1, e2
 *   - with m = world_from_object[12] of the instance the candidate counts iff
 *       tri_tri(fwd_point(m, v0), fwd_vec(m, e1), fwd_vec(m, e2), a, b, c)
 *     fwd_point and fwd_vec the functions of the box queries over a world, tri_tri the function of the triangle queries above,
 *     all unchanged, bit for bit, in float32, one rounding per operation, nothing fused. The edges are R e1 and R e2 -- not
 *     differences of posed vertices
 *   - the flat answer, which a world reproduces exactly, is taken over the ordered instance list and all leaves of every member:
 *       overlaps: d_hit[i] = 1 iff some candidate counts, else 0
 *       count: d_count[i] = the number c of candidates that count, summed over the instances (uint32)
 *       triangles: 1 <= k <= PSM_QUERY_K_MAX; rows i of d_tri and d_inst ([n][k] int32 each) hold the min(k, c) LOWEST pairs
 *         (inst, tri) that count in lexicographic order, ascending (inst and tri compared unsigned); the slots past
 *         d_count[i] = min(k, c) hold -1 in both. The row for k is a prefix of the row for any larger k; coincident instances
 *         list every shared triangle once per instance, the lowest instance first
 *   - nothing depends on the tree, its prune or the order of the walk: a flag, a sum, the lowest pairs
 *   - an identity world of one answers as psm_bvh_tri_overlaps_dev / _count_dev / _triangles_dev of its hierarchy, bit for bit
 *   - k == 0 or k > PSM_QUERY_K_MAX: PSM_ERR_INVALID, nothing is launched, as for the k-best queries. d_tris 16-byte, d_count,
 *     d_tri and d_inst 4-byte aligned, none NULL; the stale check, the depth budget, n == 0, stream order and capture as for the
 *     other world queries; an empty world answers 0 / 0 / count 0 and rows of -1 without a query kernel. A refused call
 *     launches nothing and leaves the output buffers untouched */
int psm_world_tri_overlaps_dev(psm_world* world, const psm_tri_query* d_tris, size_t n, uint8_t* d_hit);
int psm_world_tri_count_dev(psm_world* world, const psm_tri_query* d_tris, size_t n, uint32_t* d_count);
int psm_world_tri_triangles_dev(psm_world* world, const psm_tri_query* d_tris, size_t n, uint32_t k, int32_t* d_tri, int32_t* d_inst,
                                uint32_t* d_count);

/* clearance queries over a world (new; no reference counterpart): which (instance, triangle) pair of a world is
 * nearest to a triangle given in WORLD space, how far and at which two points, and whether any pair is within a radius, in one
 * launch: how much room a triangle has among the posed bodies of a world. The clearance queries against a built hierarchy with
 * the candidates of the triangle queries over a world. Flat scenes and instanced lists have no clearance query. Semantics:
 *   - a query is a psm_tri_dist_query {a, rmax, b, c} in world space and is never moved. It is valid iff its nine coordinates
 *     are finite and rmax >= 0 (NaN or negative: a miss; +inf: no limit), as for psm_bvh_tri_closest_dev; a segment or a point
 *     is a valid query. The query is not moved, so there is no per-instance validity
 *   - the candidates are the pairs (inst, tri) of the triangle queries over a world. With m = world_from_object[12] of the
 *     instance the pair's distance is
 *       tri_dist(fwd_point(m, v0), fwd_vec(m, e1), fwd_vec(m, e2), a, b, c)
 *     tri_dist the function of the clearance queries above, fwd_point and fwd_vec those of the box queries over a world, all
 *     unchanged, bit for bit, in float32. So dist == 0 exactly for the pairs psm_world_tri_overlaps_dev counts: the same tri_tri
 *     on the same eighteen numbers
 *   - the flat answer, which a world reproduces exactly: of all pairs with sqrtf(d2) <= rmax the smallest float32 d2 wins, on a
 *     bit-equal d2 the lexicographically lowest (inst, tri), both compared unsigned. closest writes psm_tri_hit {u, v, dist =
 *     sqrtf(d2), tri, s, t, 0, 0} and d_inst[i] = inst; a miss is {0, 0, +inf, -1, 0, 0, 0, 0} and -1. (u, v) weigh the STORED
 *     triangle's e1, e2 -- weights are the same for the object-space and the posed triangle: the point on the instance is
 *     (v0' + u e1') + v e2' with the posed v0', e1', e2' -- and (s, t) weigh the query's b - a, c - a
 *   - within: d_hit[i] = 1 iff closest with rmax = r finds a pair, else 0
 *   - nothing depends on the tree, its prune or the order of the walk
 *   - an identity world of one answers as psm_bvh_tri_closest_dev / psm_bvh_tri_within_dev of its hierarchy, bit for bit
 *   - d_tris and d_hits 16-byte, d_inst 4-byte aligned, none NULL; the stale check, the depth budget, n == 0, stream order and
 *     capture as for the other world queries; an empty world answers misses / 0 without a query kernel. A refused call launches
 *     nothing and leaves the output buffers untouched */
int psm_world_tri_closest_dev(psm_world* world, const psm_tri_dist_query* d_tris, size_t n, psm_tri_hit* d_hits, int32_t* d_inst);
int psm_world_tri_within_dev(psm_world* world, const psm_tri_dist_query* d_tris, size_t n, uint8_t* d_hit);

/* mesh queries over a world (new; no reference counterpart): the triangle queries over a world above with the
 * query triangles taken from a built hierarchy `other` of the world's context, at each of p rigid poses, in one call: does body
 * B, at each of these candidate poses, cut any of the bodies of the scene, which ones, and where. The mesh queries against a
 * built hierarchy with a world where `bvh` was. Nothing is downloaded, posed on the host or packed. Semantics:
 *   - other: a built hierarchy of the world's context; it may be one of the world's own members
 *   - poses: HOST memory, p x 12 floats, each a row-major 3 x 4 [R | T] that takes a point of other's object space into WORLD
 *     space (x' = R x + T), read at the call and checked as psm_instance's matrix is (finite; R^T R within 1e-5 of the identity
 *     in every entry, in double: rotations and reflections)
 *   - T = other's loaded triangle count. Outputs are indexed by pose q and by other's load-order triangle id t: d_hit [p],
 *     d_count [p][T], d_tri and d_inst [p][T][k]
 *   - the query of (pose m, triangle t of other) is that of the mesh queries, from other's STORED record, unchanged:
 *       a = fwd_point(m, v0),  b = a + fwd_vec(m, e1),  c = a + fwd_vec(m, e2)
 *     in float32, one rounding per operation, nothing fused
 *   - with skip = -1 the answer for (m, t) is BIT FOR BIT what psm_world_tri_overlaps_dev / psm_world_tri_count_dev /
 *     psm_world_tri_triangles_dev answer for psm_tri_query {a, b, c} on the same world: the candidate (inst, tri) is posed forward
 *     (R v0 + T, R e1, R e2) and judged by tri_tri; the same k rule (1 <= k <= PSM_QUERY_K_MAX), the same rows (the min(k, c)
 *     lowest (inst, tri) that count, ascending, then -1 in both arrays; d_count = min(k, c)). A query whose posed image holds a
 *     non-finite number (an overflow) meets nothing: 0, or count 0 with rows of -1
 *   - a triangle of other that its build dropped (not in PSM_BVH_LEAF_TRI) answers count 0 with rows of -1 at every pose
 *   - overlaps: d_hit[q] = 1 iff some leaf of other at pose q meets some candidate -- the OR over the pose's queries --, else 0
 *   - skip = s >= 0 leaves instance s out: the answer is that of the ordered instance list with entry s removed and the other
 *     indices KEPT ("body s at a new pose against all the others" is one call with other = its hierarchy). It is decided where
 *     an instance is entered (the lone leaf of a one-leaf member and a world of one included), never by a filter after the
 *     test: a skipped instance costs nothing. skip must be -1 or below psm_world_count()
 *   - with other a member of the world at its own pose and skip = -1, every leaf meets at least itself in that instance
 *   - nothing depends on the top-level tree, a member's tree, other's tree, the order of the walk or timing. Query i of the
 *     launch is pose i / L and other's leaf i % L by ascending triangle id (L its leaf count): the queries, in the order, of the
 *     triangle queries over a world for the same posed triangles packed in load order
 *   - refusals, all on the host before any launch and with the outputs untouched: NULL world (PSM_ERR_INVALID, no message, as
 *     every world query); then, with a message on the world's context: NULL other, poses or outputs, d_count / d_tri / d_inst
 *     not 4-byte aligned, k == 0 or k > PSM_QUERY_K_MAX (PSM_ERR_INVALID); other not built (PSM_ERR_STATE,
 *     "mesh query before build"); other of another context (PSM_ERR_INVALID); a stale world (PSM_ERR_STATE: the check and the
 *     message of every world query); a pose that is not finite or not rigid, named by its index (PSM_ERR_INVALID); skip out of
 *     range (PSM_ERR_INVALID); p x T >= 2^32 (PSM_ERR_CAPACITY)
 *   - p == 0 returns PSM_OK and touches nothing (it is answered before everything but the NULL world). Otherwise the outputs are
 *     cleared in stream order (0, rows of -1) before the one kernel; an empty world and an other without leaves launch no query
 *     kernel
 *   - the poses go to the device as the mesh queries' do: copied on the context's stream into a buffer the context owns, and the
 *     call waits for that copy (and, in the same wait, reads other's leaf count). The call therefore synchronises the context's
 *     stream ONCE before its launch and CANNOT be captured into a graph; the kernel itself is stream-ordered like every query
 *   - study knob, no part of the contract: PSM_MESH_SKIP = 0 / 1 as for the mesh queries (the overlaps kernel lets a lane skip
 *     its walk when its pose's flag already reads 1, by itself only in launches of more than PSM_QUERY_GRID_CAP waves)
 *   - not covered: mesh queries over flat scenes and instanced lists (psm_scene_*, psm_instances_*); a dual-tree walk; the
 *     intersection segments; more than one skipped instance; k > PSM_QUERY_K_MAX; graph capture of the call */
int psm_world_mesh_overlaps_dev(psm_world* world, psm_bvh* other, const float* poses, size_t p, int32_t skip, uint8_t* d_hit);
int psm_world_mesh_count_dev(psm_world* world, psm_bvh* other, const float* poses, size_t p, int32_t skip, uint32_t* d_count);
int psm_world_mesh_triangles_dev(psm_world* world, psm_bvh* other, const float* poses, size_t p, int32_t skip, uint32_t k,
                                 int32_t* d_tri, int32_t* d_inst, uint32_t* d_count);

/* mesh clearance over a world (new; no reference counterpart): "mesh clearance" above with a world where `bvh`
 * was -- how close body B comes to the other bodies of a scene at each of p candidate poses, and where. The clearance queries
 * over a world with the query triangles taken from a built hierarchy `other` of the world's context, posed on the device, and
 * the ONE nearest pair of each pose. world, other, poses, p, skip, T = other's loaded triangle count and the indexing by other's
 * load-order triangle id are those of "mesh queries over a world". Semantics:
 *   - mesh_closest: d_hits [p][T], d_inst [p][T]. The record and the instance of (pose q, triangle t of other) are BIT FOR BIT
 *     what psm_world_tri_closest_dev writes for psm_tri_dist_query {a, rmax, b, c}, with a, b, c the posed triangle exactly as
 *     the mesh queries make it (a = fwd_point(m, v0), b = a + fwd_vec(m, e1), c = a + fwd_vec(m, e2)): of all pairs (inst, tri)
 *     of the world with sqrtf(d2) <= rmax the smallest float32 d2, on a bit-equal d2 the lexicographically lowest (inst, tri).
 *     With skip = i >= 0 instance i is left out and the other indices are KEPT, decided where an instance is entered. The miss
 *     record {0, 0, +inf, -1, 0, 0, 0, 0} and instance -1 are written for a triangle that other's build dropped, for one whose
 *     posed image is not finite, and for every triangle when the world is empty
 *   - mesh_clearance: d_hits [p], one psm_mesh_hit per pose, d_inst [p]. Let t* be the lowest t among the triangles of other
 *     whose mesh_closest record has the smallest dist, comparing the float32 dist as stored. The record is that triangle's
 *     mesh_closest record, bit for bit, with other = t*, and d_inst its instance. A pose where no pair counts reads
 *     {0, 0, +inf, -1, 0, 0, -1, 0} and instance -1. (u, v) weigh e1, e2 of the instance's stored triangle tri -- the same
 *     weights on its posed image --, (s, t) weigh b - a, c - a of the posed triangle `other`: both witness points in world space
 *   - mesh_within: d_flag [p]; d_flag[q] = 1 iff mesh_clearance at rmax = r finds a pair at pose q, else 0. The walk of a
 *     triangle ends at its first pair that counts
 *   - rmax / r: one scalar per call. NaN or negative is not a refusal: it answers a miss everywhere. -0 is 0, +inf is no limit
 *   - nothing depends on the top-level tree, a member's tree, other's tree, the order of the walk or timing. Inside the
 *     clearance launch the lanes of a pose share the 64-bit word of "mesh clearance", (bits(dist) << 32) | t, t the triangle of
 *     OTHER: the word never holds the world's side of the pair, so it needs no instance. Every value it takes is the dist of a
 *     real pair that counts (never one of the skipped instance), so the final word is (the smallest dist, t*) under every
 *     schedule; a second, tiny launch of one lane per pose walks posed triangle t* again with that dist for rmax, as
 *     mesh_closest would with the same skip, and writes the record and the instance
 *   - refusals: those of the mesh queries over a world, in the same order and with the same texts under these names, all on the
 *     host before any launch and with the outputs untouched: NULL world (PSM_ERR_INVALID, no message); p == 0 returns PSM_OK and
 *     touches nothing; NULL other, poses, d_hits / d_flag or d_inst; d_hits not 16-byte aligned, d_inst not 4-byte aligned
 *     (PSM_ERR_INVALID); other not built (PSM_ERR_STATE, "mesh query before build"); other of another context
 *     (PSM_ERR_INVALID); a stale world (PSM_ERR_STATE); a pose that is not finite or not rigid, named by its index
 *     (PSM_ERR_INVALID); skip out of range (PSM_ERR_INVALID); p x T >= 2^32 (PSM_ERR_CAPACITY)
 *   - the poses go to the device as the mesh queries' do: one copy on the context's stream and ONE synchronisation before the
 *     launch (other's leaf count comes back in the same wait). The call CANNOT be captured into a graph. An empty world and an
 *     other without leaves launch no walk: the miss records (flags of 0) are written in stream order
 *   - study knobs, no part of the contract, read at each call: PSM_MESH_BOUND = 0 / 1 / 2 / 3 and PSM_MESH_SKIP = 0 / 1, with the
 *     meanings "mesh clearance" gives them; the answer is the same under each
 *   - not covered: clearance over a QueryScene or an InstancedScene; a per-pose rmax; more than one skipped instance; the k
 *     closest pairs; a dual-tree walk; penetration depth; graph capture of the call */
int psm_world_mesh_closest_dev(psm_world* world, psm_bvh* other, const float* poses, size_t p, int32_t skip, float rmax,
                               psm_tri_hit* d_hits /*[p][T]*/, int32_t* d_inst /*[p][T]*/);
int psm_world_mesh_within_dev(psm_world* world, psm_bvh* other, const float* poses, size_t p, int32_t skip, float r, uint8_t* d_flag /*[p]*/);
int psm_world_mesh_clearance_dev(psm_world* world, psm_bvh* other, const float* poses, size_t p, int32_t skip, float rmax,
                                 psm_mesh_hit* d_hits /*[p]*/, int32_t* d_inst /*[p]*/);

/* voxel grids over a built hierarchy (new; no reference counterpart): which voxels of a regular axis-aligned
 * grid a triangle overlaps (surface), how many triangles overlap each voxel (counts), and the surface with its inside filled
 * (solid) -- one call per grid, no box records: the grid is nine numbers. The answers are DEFINED by the box and inside
 * queries above, voxel by voxel and bit for bit; grid.hip gets them with one wave per 4 x 4 x 4 brick of voxels instead of one
 * lane per box. Semantics:
 *   - voxel (ix, iy, iz), 0 <= i_k < dims[k], is the closed box with, per axis k, lo_k = origin_k + (float)i_k * cell_k and
 *     hi_k = origin_k + (float)(i_k + 1) * cell_k: one float32 multiplication, then one float32 addition, nothing fused. The hi
 *     of voxel i is therefore the lo of voxel i + 1 bit for bit, and a triangle lying in that plane counts in both (the box
 *     test is closed). Its centre is c_k = origin_k + ((float)i_k + 0.5f) * cell_k
 *   - a grid is valid iff origin is finite, cell is finite and > 0, every dims[k] is in 1 .. PSM_GRID_DIM_MAX, the last voxel's
 *     hi, origin_k + (float)dims[k] * cell_k, is finite on every axis, and the brick count is below 2^31
 *   - bricks: nb_k = ceil(dims[k] / 4); brick (bx, by, bz) has index (bz * nb_y + by) * nb_x + bx and is one 64-bit word; bit
 *     j = (z & 3) * 16 + (y & 3) * 4 + (x & 3) of it is voxel (x, y, z) = (4 bx + (x & 3), 4 by + (y & 3), 4 bz + (z & 3)).
 *     Bits of voxels outside dims are 0. d_bricks holds psm_grid_brick_count(grid) = nb_x nb_y nb_z words
 *   - surface: a voxel's bit is 1 iff psm_bvh_box_overlaps_dev answers 1 for the voxel's box
 *   - counts: d_counts[(iz * ny + iy) * nx + ix] = what psm_bvh_box_count_dev answers for the voxel's box; dense, nx ny nz
 *     entries, no padding voxels
 *   - solid: a voxel's bit is its surface bit | what psm_bvh_inside_dev(centre, samples) answers, samples 1, 3 or 5 as there:
 *     for a closed mesh the filled model, for an open one merely deterministic, as inside is
 *   - nothing depends on the order of the walk or on timing: a flag, a sum
 *   - refusals, all on the host before any launch and with the output untouched: NULL bvh (PSM_ERR_INVALID, no message: there
 *     is no context to hold one); NULL grid or output; an invalid grid; d_bricks not 8-byte, d_counts not 4-byte aligned;
 *     samples not 1, 3 or 5 (PSM_ERR_INVALID); before the first build (PSM_ERR_STATE, "grid query before build"); a hierarchy
 *     deeper than the query stack (PSM_ERR_CAPACITY)
 *   - the grid is host memory, read during the call: its numbers travel as kernel arguments. The calls are stream-ordered on
 *     the hierarchy's context. surface and counts allocate nothing and can be captured into a graph. solid allocates a
 *     context-owned scratch at its first use and grows it for a larger grid (the centres and flags of at most 65 536 bricks: 68
 *     MiB, freed with the context), and its inside launches use the context's stack area, which the context's first query
 *     allocates: capture it only after a plain call with a grid at least as large
 *   - 0 leaves: all zero; 1 leaf: that leaf is tested; after psm_bvh_refit the refitted boxes are used
 *   - not covered: grids over a flat scene or an instanced list (a world has its own, "voxel grids over a world" below);
 *     conservative or 6-separating thin voxelisation; oriented grids. (The list of the non-empty bricks and the coarse level
 *     that culls empty regions before the brick walk are "voxel grids: sparse" below) */
#define PSM_GRID_DIM_MAX (1u << 20)
typedef struct {
    float origin[3];   /* corner of voxel (0, 0, 0) */
    float cell[3];     /* voxel size per axis, > 0 */
    uint32_t dims[3];  /* nx, ny, nz, each >= 1 */
} psm_grid;            /* host memory, read during the call */
int psm_grid_surface_dev(psm_bvh* bvh, const psm_grid* grid, uint64_t* d_bricks);
int psm_grid_counts_dev(psm_bvh* bvh, const psm_grid* grid, uint32_t* d_counts);
int psm_grid_solid_dev(psm_bvh* bvh, const psm_grid* grid, uint32_t samples, uint64_t* d_bricks);
uint64_t psm_grid_brick_count(const psm_grid* grid);   /* 0 for an invalid grid (NULL too); host only */

/* voxel grids: distance fields (new; no reference counterpart): the distance from every voxel centre of a
 * psm_grid to the nearest triangle within rmax, and that triangle's id -- one call per grid, no point records. The answers are
 * DEFINED by the point queries above, voxel by voxel and bit for bit; grid_dist.hip gets them with one wave per 4 x 4 x 4 brick,
 * which walks the tree once for its 64 centres. psm_grid, its validity rules and the centre are those of "voxel grids".
 * Semantics:
 *   - d_dist[(iz * ny + iy) * nx + ix] (float32) is bit for bit the t psm_bvh_closest_point_dev writes for {centre, rmax}: +inf
 *     when no triangle lies within rmax. d_tri (int32, same index) is that record's tri, the load-order id; on a bit-equal
 *     squared distance the lowest id wins; -1 on a miss. Both dense, nx ny nz entries, no padding voxels. d_tri may be NULL: the
 *     ids are then not stored
 *   - signed: d_dist is bit for bit the t of psm_bvh_signed_distance_dev for {centre, rmax} with `samples` rays: the sign bit
 *     is set iff the voxel has a record and psm_bvh_inside_dev(centre, samples) holds (-0 can occur); a voxel with no record
 *     stays +inf, sign bit clear, and casts no rays. d_tri is unchanged by the sign
 *   - u, v and the closest point itself are not written: psm_bvh_closest_point_dev answers them for the voxels that need them
 *   - rmax must be >= 0 or +inf (-0 is 0); NaN or a negative rmax is refused, it does not become a grid of misses
 *   - nothing depends on the order of the walk or on timing: a minimum with the lowest id on ties
 *   - refusals, all on the host before any launch and with the outputs untouched, in this order: NULL bvh (PSM_ERR_INVALID, no
 *     message); NULL grid or d_dist; an invalid grid; d_dist or d_tri not 4-byte aligned; rmax ("rmax must be >= 0"); samples
 *     not 1, 3 or 5 (signed only; all PSM_ERR_INVALID); before the first build (PSM_ERR_STATE, "grid query before build"); a
 *     hierarchy deeper than the query stack (PSM_ERR_CAPACITY)
 *   - stream-ordered on the hierarchy's context. psm_grid_distance_dev allocates nothing and can be captured into a graph.
 *     psm_grid_signed_distance_dev works a slab of at most 32 768 bricks at a time (the centres, the records, the sign kernel
 *     of psm_bvh_signed_distance_dev over both, the records into the dense arrays) in solid's context-owned scratch, which it
 *     allocates at its first use and grows for a larger grid (solid's 68 MiB at most, freed with the context); its sign launches use
 *     the context's stack area, which the context's first query allocates
 *   - 0 leaves: all +inf / -1; 1 leaf: that leaf is tested; after psm_bvh_refit the refitted boxes are used
 *   - not covered: distance grids over a flat scene or an instanced list (a world has its own, "voxel grids over a world:
 *     distance fields" below); u, v and the closest point per voxel; a per-voxel rmax; sweeping-based
 *     (approximate) distance transforms; graph capture of the signed call. (The band's bricks alone: "voxel grids: sparse") */
int psm_grid_distance_dev(psm_bvh* bvh, const psm_grid* grid, float rmax, float* d_dist /*[nz][ny][nx]*/, int32_t* d_tri /*[nz][ny][nx] or NULL*/);
int psm_grid_signed_distance_dev(psm_bvh* bvh, const psm_grid* grid, float rmax, uint32_t samples, float* d_dist, int32_t* d_tri);

/* voxel grids: sparse (new; no reference counterpart): which 4 x 4 x 4 bricks of a psm_grid hold anything at
 * all, as an ascending list, and the surface words or the (signed) distances of the bricks of a list -- a narrow band costs
 * its own bricks, not the grid's. Everything is DEFINED by the dense calls above, bit for bit; psm_grid, its validity rules,
 * the brick index (bz * nby + by) * nbx + bx and the bit / lane order j = (z & 3) * 16 + (y & 3) * 4 + (x & 3) are those of
 * "voxel grids".
 * Listing (the two *_bricks_dev calls):
 *   - the surface call lists brick b iff word b of psm_grid_surface_dev is non-zero; the distance call lists b iff some voxel
 *     of b has a record in psm_grid_distance_dev(rmax), tri >= 0 (closed: a centre at exactly rmax counts)
 *   - *d_count is the number of such bricks in the whole grid, also when it exceeds capacity; d_ids gets the first
 *     min(count, capacity) of them in ascending index, the slots past that are untouched. capacity 0 with d_ids NULL counts only
 *   - the list is the same under every schedule: the compaction is an ordered scan (a count per 1 024 bricks, one workgroup's
 *     scan, a scatter by rank), not an atomic append
 *   - rmax as the dense rules have it; with +inf every brick of a mesh with a leaf is listed. 0 leaves: count 0
 *   - how: a coarse pass, one lane per brick, drops the bricks the tree proves empty (the brick's whole box, or its centre
 *     with rmax widened by the farthest centre's offset and a slack: conservative); the rest are walked as the
 *     dense kernels walk them, one wave a brick, left at the first hit. PSM_SPARSE_COARSE = 0 (the environment, read at each
 *     call; a study knob, no part of the contract) and rmax = +inf skip the coarse pass; the list is the same
 * Filling (the other three):
 *   - slot i answers brick d_ids[i]: d_words[i] is the dense surface word; d_dist[i * 64 + j] and d_tri[i * 64 + j] are the
 *     dense dist and tri of the voxel at lane j. A lane outside dims holds +inf / -1: the sparse arrays have these padding
 *     lanes, 64 a brick always, where the dense arrays have none. d_tri may be NULL
 *   - an id at or above the grid's brick count is an empty brick: word 0, all +inf / -1; nothing is read or written out of
 *     range. Duplicates are allowed, any order, any list: last step's band dilated, say. n == 0 is PSM_OK, nothing launched
 *   - signed: psm_bvh_signed_distance_dev's sign kernel over the listed bricks' records, in slabs of at most 32 768 bricks of
 *     the list in the scratch of "voxel grids"; a lane with no record casts no ray
 * Refusals, all on the host before any launch and with the outputs untouched: those of the dense calls in their order and
 * texts, the output they name being d_count, d_words or d_dist and the alignment that of every pointer passed (4 bytes, the
 * words 8); then, after the hierarchy's state, a NULL d_ids with capacity > 0 or n > 0 (PSM_ERR_INVALID, "NULL pointer") and a
 * grid of more than PSM_GRID_SPARSE_BRICKS_MAX bricks (PSM_ERR_CAPACITY; 2^27: a 2048^3 grid).
 * Scratch: the listing calls keep a byte per brick, 4 bytes per 1 024 bricks, the candidates' count and -- with the coarse
 * pass -- 4 bytes per brick of candidate ids in a context-owned area: at most 5 bricks + 4 ceil(bricks / 1024) + 768 bytes,
 * 671 613 696 at the cap, 10.5 MB for a 512^3 grid; grown on demand, freed with the context. The listing calls and the two
 * unsigned filling calls make no host synchronisation -- the candidates' count stays on the device, and the waves stride
 * over it under PSM_QUERY_GRID_CAP -- and the unsigned filling calls allocate nothing: those two can always be captured into a
 * graph, the listing calls after a plain call with a grid of at least as many bricks (and the same coarse setting). The
 * signed filling call is not capturable, as the dense signed call.
 * Not covered: sparse grids over a world; sparse counts or solid; bricks other than 4^3; a tree of bricks; dilating or
 * eroding a list. */
#define PSM_GRID_SPARSE_BRICKS_MAX (1u << 27)
int psm_grid_sparse_surface_bricks_dev(psm_bvh* bvh, const psm_grid* grid, uint32_t capacity, uint32_t* d_ids /*[capacity] or NULL when capacity == 0*/,
                                       uint32_t* d_count);
int psm_grid_sparse_distance_bricks_dev(psm_bvh* bvh, const psm_grid* grid, float rmax, uint32_t capacity, uint32_t* d_ids, uint32_t* d_count);
int psm_grid_sparse_surface_dev(psm_bvh* bvh, const psm_grid* grid, const uint32_t* d_ids, uint32_t n, uint64_t* d_words /*[n]*/);
int psm_grid_sparse_distance_dev(psm_bvh* bvh, const psm_grid* grid, float rmax, const uint32_t* d_ids, uint32_t n, float* d_dist /*[n][64]*/,
                                 int32_t* d_tri /*[n][64] or NULL*/);
int psm_grid_sparse_signed_distance_dev(psm_bvh* bvh, const psm_grid* grid, float rmax, uint32_t samples, const uint32_t* d_ids, uint32_t n,
                                        float* d_dist, int32_t* d_tri);

/* voxel grids over a world (new; no reference counterpart): the grids above over the posed instances of a
 * psm_world -- the occupancy map of an assembled scene whose bodies move by a matrix per step --, and which body owns each
 * voxel. psm_grid, its validity rules, the voxel box, the centre, the brick layout and psm_grid_brick_count are those of "voxel
 * grids"; the grid is a WORLD grid and is never moved. The answers are DEFINED by the world's box and inside queries, voxel by
 * voxel and bit for bit; world_grid.hip gets them with one wave per 4 x 4 x 4 brick, which walks the tree over the instances and
 * the hierarchies it enters once for its 64 voxels. Semantics:
 *   - surface: a voxel's bit is 1 iff psm_world_box_overlaps_dev answers 1 for the voxel's box; one 64-bit word per brick,
 *     the bits of voxels outside dims 0, exactly psm_grid_surface_dev's layout
 *   - counts: d_counts[(iz * ny + iy) * nx + ix] = what psm_world_box_count_dev answers for the voxel's box: the number of
 *     (instance, triangle) pairs; dense, nx ny nz entries
 *   - instances (the owner): d_inst[(iz * ny + iy) * nx + ix] = slot 0 of the instance row psm_world_box_triangles_dev(k = 1)
 *     answers for the voxel's box: the lowest instance index that has a counting triangle, -1 for none; dense int32
 *   - solid: a voxel's bit is its surface bit | what psm_world_inside_dev(centre, samples) answers, samples 1, 3 or 5
 *   - nothing depends on the order of the walk or on timing: a flag, a sum, a minimum
 *   - refusals, all on the host before any launch and with the output untouched, in this order: NULL world (PSM_ERR_INVALID, no
 *     message: there is no context to hold one); NULL grid or output; an invalid grid ("<name>: invalid grid: <why>"); d_bricks
 *     not 8-byte, d_counts or d_inst not 4-byte aligned; samples not 1, 3 or 5 (PSM_ERR_INVALID). Then an empty world is answered
 *     in stream order without a query kernel: zero words, zero counts, -1 labels. Then a world one of whose hierarchies was
 *     rebuilt after psm_world_set_instances is refused as by every world query (PSM_ERR_STATE). The depth rule is
 *     psm_world_set_instances': a world that was accepted fits the wave's one stack
 *   - the grid is host memory, read during the call. The calls are stream-ordered on the world's context. surface, counts and
 *     instances allocate nothing and can be captured into a graph. solid runs the surface launch and then, per slab of at most
 *     65 536 bricks, the centres, psm_world_inside_dev and the fill, with the context-owned scratch and the stack area of "voxel
 *     grids"
 *   - not covered: grids over a flat scene or an instanced list; the skip of one instance; per-voxel lists of more than one
 *     instance; a sparse output; a coarse level that culls empty bricks before the walk; oriented grids;
 *     graph capture of solid (the signed-distance grid of a world is the next section's) */
int psm_grid_world_surface_dev(psm_world* world, const psm_grid* grid, uint64_t* d_bricks);
int psm_grid_world_counts_dev(psm_world* world, const psm_grid* grid, uint32_t* d_counts);
int psm_grid_world_instances_dev(psm_world* world, const psm_grid* grid, int32_t* d_inst);
int psm_grid_world_solid_dev(psm_world* world, const psm_grid* grid, uint32_t samples, uint64_t* d_bricks);

/* voxel grids over a world: distance fields (new; no reference counterpart): the distance from every voxel
 * centre of a psm_grid to the nearest posed triangle of any instance of a psm_world within rmax, that triangle's id and its
 * instance -- a planner's clearance map, or with the sign a narrow-band signed-distance grid, over bodies that each move by a
 * matrix per step; one call per grid, no point records. psm_grid, its validity rules and the centre are those of "voxel
 * grids"; the grid is a WORLD grid and is never moved. The answers are DEFINED by the world's point queries, voxel by voxel and
 * bit for bit; world_grid_dist.hip gets them with one wave per 4 x 4 x 4 brick, which walks the tree over the instances and the
 * hierarchies it enters once for its 64 centres. Semantics:
 *   - d_dist[(iz * ny + iy) * nx + ix] (float32) is bit for bit the t psm_world_closest_point_dev writes for {centre, rmax}:
 *     +inf when no triangle lies within rmax. d_tri (int32, same index) is that record's tri, d_inst (int32, same index) its
 *     instance; -1 in both on a miss. On a bit-equal squared distance the lexicographically lowest (instance, triangle) wins.
 *     All dense, nx ny nz entries, no padding voxels. d_tri and d_inst may each be NULL: they are then not stored
 *   - signed: d_dist is bit for bit the t of psm_world_signed_distance_dev for {centre, rmax} with `samples` rays: the sign bit
 *     is set iff the voxel has a record and psm_world_inside_dev(centre, samples) holds -- the parity summed over all
 *     instances (-0 can occur); a voxel with no record stays +inf, sign bit clear, and casts no rays. d_tri and d_inst are
 *     unchanged by the sign
 *   - u, v and the closest point itself are not written: psm_world_closest_point_dev answers them for the voxels that need them
 *   - rmax must be >= 0 or +inf (-0 is 0); NaN or a negative rmax is refused, it does not become a grid of misses
 *   - nothing depends on the order of the walk or on timing: a minimum with the lowest (instance, triangle) on ties
 *   - refusals, all on the host before any launch and with the outputs untouched, in this order: NULL world (PSM_ERR_INVALID, no
 *     message: there is no context to hold one); NULL grid or d_dist; an invalid grid ("<name>: invalid grid: <why>"); d_dist,
 *     d_tri or d_inst not 4-byte aligned; rmax ("rmax must be >= 0"); samples not 1, 3 or 5 (signed only; all PSM_ERR_INVALID).
 *     Then an empty world is answered in stream order by fills alone, without a query kernel: +inf, -1, -1. Then a world one of
 *     whose hierarchies was rebuilt after psm_world_set_instances is refused as by every world query (PSM_ERR_STATE). The depth
 *     rule is psm_world_set_instances': a world that was accepted fits the wave's one stack
 *   - the grid is host memory, read during the call. Stream-ordered on the world's context. psm_grid_world_distance_dev
 *     allocates nothing and can be captured into a graph. psm_grid_world_signed_distance_dev works a slab of at most 32 768
 *     bricks at a time (the centres, the walk's records, the sign kernel of psm_world_signed_distance_dev over both, the
 *     records into the dense arrays; the instances are written by the walk) in the context-owned scratch of "voxel grids",
 *     32 bytes a voxel, and its sign launches use the context's stack area
 *   - instances of 0-leaf hierarchies hold nothing; a 1-leaf hierarchy's leaf is tested; after psm_bvh_refit and
 *     psm_world_set_transforms over the whole range the refitted boxes are used
 *   - not covered: distance grids over a flat scene or an instanced list; the skip of one instance; a per-voxel rmax; a sparse
 *     output; graph capture of the signed call */
int psm_grid_world_distance_dev(psm_world* world, const psm_grid* grid, float rmax, float* d_dist /*[nz][ny][nx]*/,
                                int32_t* d_tri /*same, or NULL*/, int32_t* d_inst /*same, or NULL*/);
int psm_grid_world_signed_distance_dev(psm_world* world, const psm_grid* grid, float rmax, uint32_t samples, float* d_dist,
                                       int32_t* d_tri, int32_t* d_inst);

/* ---------------------------------------------------------------------------------------------
 * several frames in flight (new; DESIGN.md "lanes")
 * `frames` x GltfViewer::process() (Viewer.cpp:296-312) with up to `lanes` of them in flight: lane s =
 * (rts[s], bvhs[s]) on its own context / stream. Frame f has its own CRT-rand() stand-in, started from
 * frame_seeds[f] (one draw for camera(), one per shade(), as Pipeline.inl:282,426 draw them) and runs: build (if
 * rebuild != 0, with `opt`), camera, at most `depth` rounds of { stop if fewer than 32 rays (Pipeline.inl:459-461);
 * intersection; shade }, then sample() -- issued on `fold_into` (psm_rt_sample_from) in frame order, so the
 * accumulated image equals the frames rendered one after another. Lanes never wait for each other's rounds: a
 * frame's traversal tail overlaps the other frames' kernels, and a lane takes the next frame as soon as its own is
 * folded. fold_into may be NULL when frames <= lanes (the lanes then keep their frames for the caller to fold).
 * Materials / lights / sky / textures / tiles must have been set on every rt. One hierarchy per lane: frames that
 * intersect several hierarchies (multi-BVH) go through the per-call API. Returns when everything is idle.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    uint32_t rounds; /* shade() calls made for this frame */
    uint64_t rays;   /* rays traced */
} psm_lane_result;
int psm_lanes_render(psm_rt* const* rts, psm_bvh* const* bvhs, uint32_t lanes, const float cam_inv[16],
                     const float proj_inv[16], const uint32_t* frame_seeds, uint32_t frames, uint32_t depth,
                     int rebuild, const double* opt, psm_rt* fold_into, psm_lane_result* results /* [frames] */);
/* The same frames when they are tile-sharded over several GPUs: the `fewer than 32 rays -> stop` rule then looks
 * at each frame's GLOBAL count. A rank with >= 32 local rays knows the global count is >= 32 too, so every lane
 * runs free (as above) until its LOCAL count drops below 32 or `depth` is reached, and then parks with its queue
 * intact. Returns when all lanes are parked: rounds[s] = rounds done, counts_out[s] = local rays waiting. The host
 * exchanges those (one small all-gather per batch as a rule: the tiles of a frame run dry in the same round) and,
 * where a frame's global count says it goes on, calls again with start = 0 and force_until[s] = the round lane s
 * must reach whatever its local count (it traces its few rays, or none, drawing its rand() every round so the
 * ranks stay in step). start != 0 begins new frames: build (if rebuild) + camera, rounds[] reset.
 * rand_state[s]: the frame's CRT-rand() stand-in state, in/out across calls. */
int psm_lanes_run_sharded(psm_rt* const* rts, psm_bvh* const* bvhs, uint32_t lanes, const float cam_inv[16],
                          const float proj_inv[16], uint32_t* rand_state, uint32_t* rounds, const uint32_t* force_until,
                          uint32_t depth, int start, int rebuild, const double* opt, int32_t* counts_out);

/* ---------------------------------------------------------------------------------------------
 * tile-sharded frames across the GPUs of one node (new; SURVEY 8(b) "proposed C ABI", 8(e); the reference has no
 * multi-GPU path). One process per GPU. The path has ONE data-path collective per frame: the gather of every tile's
 * per-texel radiance to rank 0 (RCCL over xGMI), which runs sample() on the whole image. psm_dist_allgather_i32
 * carries the (round, ray count) pairs psm_lanes_run_sharded asks the host to exchange.
 *   rank 0:   psm_dist_unique_id(id);  ... hand `id` to the other ranks (any side channel) ...
 *   all:      psm_dist_init(ctx, rank, world, id, &dist);  psm_rt_set_tile_interleaved(rt, rank, world);
 *   a frame:  camera / rounds on rt ...; psm_dist_gather_tiles(dist, rt);  rank 0: psm_rt_sample(rt)
 * Every rank makes the same psm_dist_* calls in the same order. Collectives run on the communicator's own stream,
 * ordered against the Pipeline's stream by events: no host synchronisation in psm_dist_gather_tiles.
 * ------------------------------------------------------------------------------------------- */
typedef struct psm_dist psm_dist;
int psm_dist_unique_id(uint8_t id[128]);                        /* ncclGetUniqueId */
int psm_dist_init(psm_ctx* ctx, int rank, int world, const uint8_t id[128], psm_dist** out); /* ncclCommInitRank on ctx's device; collective */
/* The same in two steps, for launchers that want to agree between them: psm_dist_prepare creates this rank's LOCAL
 * resources only (stream, events; cannot block on a peer), psm_dist_connect is the collective ncclCommInitRank. A rank
 * whose prepare failed can tell the others over the side channel before anybody is inside the collective. */
int psm_dist_prepare(psm_ctx* ctx, int rank, int world, psm_dist** out);
int psm_dist_connect(psm_dist* dist, const uint8_t id[128]);
/* The transport seam: the two exchanges of the path as a table of functions. psm_dist_init / psm_dist_connect install
 * RCCL (ncclGather / ncclAllGather on the communicator's stream, stream-ordered); psm_dist_connect_transport installs
 * the caller's table instead, and psm_dist_connect_hoststaged a transport built into the library that stages through a
 * POSIX shared-memory segment (hipMemcpy to the host, sequence counters, bounded waits), so that several processes
 * SHARING ONE GPU -- which RCCL refuses -- can drive the whole sharded scheduler against real peers (tests; never
 * chosen silently). A transport function returns 0 or non-zero; it may complete on `hip_stream` (a hipStream_t) or
 * synchronously on the host. All pointers are device pointers. */
typedef struct {
    void* user;
    /* `count` floats of every rank at d_send -> root's d_recv[world * count] in rank order (d_recv is NULL elsewhere) */
    int (*gather_f32)(void* user, const float* d_send, float* d_recv, size_t count, int root, void* hip_stream);
    /* n ints of every rank at d_send -> every rank's d_recv[world * n] in rank order */
    int (*allgather_i32)(void* user, const int32_t* d_send, int32_t* d_recv, size_t n, void* hip_stream);
    void (*destroy)(void* user);            /* may be NULL */
    const char* (*last_error)(void* user);  /* may be NULL */
    const char* name;                       /* e.g. "rccl", "host-staged" */
} psm_dist_transport;
int psm_dist_connect_transport(psm_dist* dist, const psm_dist_transport* transport);
/* shm_name: a POSIX shared-memory name every rank of the group passes ("/psm-<unique>"); rank 0 creates it and unlinks
 * it once all ranks are attached. slot_bytes >= the largest tile of a gather (16 B x the texels rank 0 owns);
 * timeout_ms bounds every wait for a peer (PSM_ERR_PEER afterwards, on every rank that waits). */
int psm_dist_connect_hoststaged(psm_dist* dist, const char* shm_name, size_t slot_bytes, uint32_t timeout_ms);
const char* psm_dist_transport_name(const psm_dist* dist);     /* NULL while not connected */
int psm_dist_destroy(psm_dist* dist);
int psm_dist_rank(const psm_dist* dist);
int psm_dist_world(const psm_dist* dist);
/* the ranks the TRANSPORT itself counts in the communicator -- RCCL: ncclCommCount (psm_dist_connect fails unless it equals `world`
 * and ncclCommUserRank equals `rank`); host-staged: the processes attached to the segment; 0 while not connected. What a bench line
 * should print next to n_gpus. */
int psm_dist_comm_ranks(const psm_dist* dist);
/* pack rt's owned texels, ncclGather them to rank 0, and there unpack the tiles of ranks 1..world-1 into rt's image
 * (rt must carry psm_rt_set_tile_interleaved(rank, world) of this communicator). 16 B per texel; 1080p: 33 MB in all. */
int psm_dist_gather_tiles(psm_dist* dist, psm_rt* rt);
/* n ints from every rank to every rank (host arrays: recv holds world * n); synchronises */
int psm_dist_allgather_i32(psm_dist* dist, const int32_t* send, int32_t* recv, uint32_t n);
int psm_dist_barrier(psm_dist* dist);
/* every rank's own status (PSM_OK or its error code) -> one verdict for all: PSM_OK when every rank is fine, this rank's
 * own code when it failed, PSM_ERR_PEER when only others did. One one-int all-gather; every rank must call it. */
int psm_dist_agree(psm_dist* dist, int local_rc);
/* the global `fewer than 32 rays -> stop` rule (Pipeline.inl:459-461) from every rank's answers: all = [world][2][lanes]
 * (rounds done, local rays waiting) as gathered after psm_lanes_run_sharded -> per lane: over (the frame has ended) and
 * force_until (the round every rank must reach next). Pure host arithmetic; needs no device.
 * A rank that failed locally reports rounds = -1 for its lanes (it keeps taking part in the collectives so that nobody
 * waits for it): any negative round makes psm_dist_decide return PSM_ERR_PEER on every rank at the same exchange. */
int psm_dist_decide(uint32_t world, uint32_t lanes, const int32_t* all, uint32_t depth, int32_t* over, uint32_t* force_until);
/* `lanes` tile-sharded frames in flight, start to finish, on this rank (every rank makes the same call): build (if
 * rebuild) + camera + rounds on lanes that run free and park on their local counts (psm_lanes_run_sharded), the
 * all-gathers + psm_dist_decide until every frame has ended, then per frame, in frame order, psm_dist_gather_tiles and on
 * rank 0 psm_rt_sample_from(fold_into, lane). rts[s] must carry psm_rt_set_tile_interleaved(rank, world); fold_into is
 * rank 0's accumulating Pipeline (ignored elsewhere); rounds_out[lanes] may be NULL.
 * Failure: a rank whose own work fails (build, kernels, capacity) keeps the collective sequence -- it reports rounds = -1
 * at the next exchange and sends an empty tile to gathers already due -- so every rank leaves at the same exchange
 * with an error (its own, or PSM_ERR_PEER) instead of waiting inside a collective; a last one-int exchange makes the
 * return code agree when the failure came after the last decision. Only a failing transport call itself cannot be
 * covered. */
int psm_dist_render_batch(psm_dist* dist, psm_rt* const* rts, psm_bvh* const* bvhs, uint32_t lanes, const float cam_inv[16],
                          const float proj_inv[16], const uint32_t* frame_seeds, uint32_t depth, int rebuild, const double* opt,
                          psm_rt* fold_into, uint32_t* rounds_out);
/* `frames` tile-sharded frames with `lanes` of them in flight and NO drain between batches: the lanes form two groups
 * that alternate batches of lanes / 2 frames -- while one group exchanges, gathers and folds, the other group's frames
 * keep the chip busy -- with the same collective sequence on every rank (one communicator). Same arguments and result
 * as psm_dist_render_batch called ceil(frames / lanes) times; frame_seeds[frames], rounds_out[frames] or NULL. */
int psm_dist_render_frames(psm_dist* dist, psm_rt* const* rts, psm_bvh* const* bvhs, uint32_t lanes, const float cam_inv[16],
                           const float proj_inv[16], const uint32_t* frame_seeds, uint32_t frames, uint32_t depth, int rebuild,
                           const double* opt, psm_rt* fold_into, uint32_t* rounds_out);
/* one-GPU rehearsal of a worker rank's per-frame cost: gathers pack tile (tile_rank, tile_world) instead of the
 * communicator's own (rank, world) and unpack nothing (the image is then not a complete frame) */
int psm_dist_emulate_tile(psm_dist* dist, int tile_rank, int tile_world);
/* the dealing of the bands this communicator's gathers pack and unpack (psm_rt_set_tile_weighted's weights; NULL =
 * round-robin, the default). Every rank passes the same weights. */
int psm_dist_set_band_weights(psm_dist* dist, const uint32_t* weights);

/* ---------------------------------------------------------------------------------------------
 * statistics (PROFILE_RT replacement, Utils.hpp:27): algorithmic counters + HIP-event timing
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    uint64_t rays_traced;     /* R: rays handed to traverse since reset */
    uint64_t node_visits;     /* V (only counted while counting is enabled) */
    uint64_t tri_tests;       /* T */
    uint64_t stack_drops, iter_caps, baked_drops, chain_pool_drops, ray_limit_drops;
                              /* chain_pool_drops: equal-distance chains cut to their head because the chain pool (currentRayLimit / 2
                               * entries beside one head per ray; Pipeline.inl:193) was full */
    uint32_t traverse_launches;
    float traverse_ms;        /* sum of HIP-event durations of the traverse kernel */
    float build_ms, sort_ms, shade_ms, camera_ms, sample_ms;
    uint32_t rounds;
    float bounds_ms, morton_ms, emit_ms; /* parts of build_ms: minmax + fit, Morton codes + leaves, node emission + link + refit */
    /* clock diagnosis, counted with V and T: over all traversal waves, the sums of their lifetimes in shader-clock ticks
     * (s_memtime) and in ticks of the constant 100 MHz clock (s_memrealtime) -- their ratio x 100 MHz is the clock the chip
     * held while they ran -- the wave-steps they took and their number */
    uint64_t wave_clock_ticks, wave_real_ticks, wave_steps, waves;
    /* the part of traverse_launches / traverse_ms that are launches of the hand-over kernel (rt_traverse<*, false, true>:
     * the PHASED / ADAPTIVE schedules, what AUTO runs with frames in flight); the rest are single-launch traversals */
    uint32_t handover_launches;
    float handover_ms;
} psm_stats;
/* timing: 0 off; 1 HIP events around every launch, per stage (the rebuild then runs as plain launches instead of its
 * captured graph); 2 traversal launches only -- light enough to stay on while frames are in flight, the build keeps
 * its graph. counting: V, T and the drop counters (the counting instantiations of the kernels). */
int psm_stats_enable(psm_ctx* ctx, int timing, int counting);
int psm_stats_reset(psm_ctx* ctx);
/* one time axis for the traversal launches of several contexts of a device (frames in flight): psm_stats_reference(ctx,
 * ctx) records the origin on ctx's stream, psm_stats_reference(other, ctx) makes `other` share it (the origin context must
 * outlive the sharing ones' next reference); psm_stats_traverse_intervals then returns start, end in ms after the origin of
 * every traversal launch timed since the last reset (start_end_ms[2 * cap_launches], *count = launches recorded) */
int psm_stats_reference(psm_ctx* ctx, psm_ctx* origin);
int psm_stats_traverse_intervals(psm_ctx* ctx, float* start_end_ms, uint32_t cap_launches, uint32_t* count);
int psm_stats_get(psm_ctx* ctx, psm_stats* out); /* synchronises */

#ifdef __cplusplus
}
#endif
#endif /* PSM_HIP_H */
