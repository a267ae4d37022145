/*
 * art.h -- C ABI of libart, the MI355X-native (gfx950, HIP) ray-tracing core that stands in for the Vulkan
 * ray-tracing path of EdoardoLuciani/ARayTracingJourney.
 *
 * The reference has no FFI of its own: the path sits behind Rust methods that record Vulkan commands.  Each entry
 * point below names the reference interface (path:line under /root/reference/src/vk_renderer/) it replaces; the
 * binding a maintainer of the reference would add (a Rust `extern "C"` block) is shown in INTEGRATION.md.
 *
 * Conventions
 *  - every function returns 0 on success or a negative ART_E_* code; art_last_error() gives a thread-local message;
 *    nothing throws or unwinds across the boundary (the reference panics instead: renderer.rs uses unwrap/expect);
 *  - a context is single-threaded, like the reference's Rc<RefCell<..>> objects (renderer.rs:122-126);
 *  - plain pointers and sizes only; device work is enqueued on one HIP stream per context and art_sync() is the
 *    fence (the reference's analogue is the per-frame VkFence, renderer.rs:451-466);
 *  - there is NO CPU fallback: every compute entry point fails with ART_E_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef ART_H
#define ART_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ART_OK 0
#define ART_E_INVALID (-1)    /* bad argument */
#define ART_E_STATE (-2)      /* call out of order (e.g. trace before scene build) */
#define ART_E_NO_DEVICE (-3)  /* no HIP device / kernels not loadable */
#define ART_E_HIP (-4)        /* HIP runtime error, see art_last_error() */
#define ART_E_NOMEM (-5)

/* 48-byte interleaved vertex: model_reader.rs:22-35, gltf_model_reader.rs:176-199, raytrace.rgen.glsl:39-50 */
typedef struct ArtVertex {
    float pos[3];
    float uv[2];
    float normal[3];
    float tangent[4];
} ArtVertex;

/* 80-byte light record: lights.rs:69-82 (LightShaderData) == light.glsl:1-12 (Light) */
typedef struct ArtLight {
    float pos[3];
    uint32_t type; /* 0 point, 1 spot, 2 directional, 3 area (lights.rs:88-93) */
    float dir[3];
    uint32_t casts_shadows;
    float color[3];
    float falloff_distance;
    float area_pos2[3];
    float penumbra_angle;
    float area_pos3[3];
    float umbra_angle;
} ArtLight;

/* 268-byte camera block: vk_camera.rs:9-16 (Uniform) == raytrace.rgen.glsl:29-35; column-major mat4 */
#pragma pack(push, 1)
typedef struct ArtCamera {
    float view[16];
    float view_inv[16];
    float proj[16];
    float proj_inv[16];
    float camera_pos[3];
} ArtCamera;
#pragma pack(pop)

typedef struct ArtConfig {
    int32_t device;       /* HIP device ordinal; -1 = current device */
    uint32_t width;       /* initial extent (renderer.rs:140 takes vk::Extent2D) */
    uint32_t height;
    uint32_t morton_bits; /* 30 or 63; 0 = default (63) */
    uint32_t shard_rank;  /* screen-tile sharding: this context renders the 32x32 tiles owned by shard_rank of */
    uint32_t shard_count; /*   shard_count (0 or 1 = whole frame) */
    uint32_t flags;       /* ART_FLAG_* */
    uint32_t frames_in_flight; /* 0|1 = one; up to 24 (more than ~22 streams stall the command processor): a ring of per-frame streams + buffers like the reference's FrameData
                                  ring (renderer.rs:135, :300-318); art_trace then returns while up to N-1 older frames run */
    uint32_t root_relief;      /* sharded contexts, 0..255 (default 0 = equal shares), the same on every rank of a job: shard 0 -- the rank that also receives and un-tiles
                                  every frame when frames are assembled on rank 0 -- gives up its tile in root_relief / 256 of the tile groups to the other shards in turn, so
                                  that its share + compositing takes as long as the others' shares (art_shard_layout takes the same value) */
} ArtConfig;

#define ART_FLAG_FAST_BUILD 2u /* traversal nodes keep the LBVH topology (PREFER_FAST_BUILD); default: binned-SAH rebuild = PREFER_FAST_TRACE, vk_model.rs:968 */
#define ART_FLAG_PACKED_TILES 4u /* sharded contexts: the compact tile buffer (the gather's payload) holds B10G11R11_UFLOAT_PACK32 words -- the reference's colour
                                   image format (renderer.rs:268) -- 4 B per pixel instead of RGB32F's 12; art_untile_gathered then assembles the packed colour image */
/* (flag bit 8 was ART_FLAG_DEVICE_TREE until round 4 -- a PLOC-built tree, superseded by the binned SAH on the device: ignored) */
#define ART_FLAG_FIXED_WAVES 16u /* every 8x8 pixel block of a frame is traced by one wave, always.  Default: adaptive -- now and then a frame counts the packet
                                  * steps of each of its waves, and blocks whose wave outlasts the launch's fair share of the GPU (a packet crossing dense distant
                                  * geometry) are dealt to 4 or 16 waves in the following frames.  The image does not depend on it. */
#define ART_FLAG_TILE_OUTPUT 32u /* write the compact tile buffer even when the frame is not sharded (shard_count <= 1: one shard owning every tile): a job of ONE rank
                                  * then runs the whole art_mgpu_* path -- gather from itself, un-tile -- which is how the RCCL transport is exercised on a one-GPU machine */
#define ART_FLAG_DYNAMIC_SCENE 64u /* the host will move models (art_scene_set_model_matrix) or switch them in and out (art_scene_set_primitive_enabled): art_scene_build also makes the
                                   * ring of structure versions a refit writes into (ArtStats.first_move_ms otherwise falls into the first frame after the first move) */
#define ART_FLAG_KEEP_DEBUG 1u /* keep per-pixel hit records / shadow bits readable (art_read_hits, art_read_shadow_bits: include/art_parity.h) */

typedef struct ArtStats {
    uint64_t primary_rays;      /* W*H of the pixels this context owns */
    uint64_t shadow_rays;       /* shadow rays actually traced: hit && casts_shadows && N.L > 0 (raytrace.rgen.glsl:165) */
    uint64_t hit_pixels;
    uint64_t ao_rays;
    uint32_t num_triangles;
    uint32_t num_primitives;
    uint32_t num_nodes;         /* nodes of the traversal structure */
    uint32_t frame_launches; /* kernel launches per frame: 1 = fused frame kernel, 4 = primary / shade / shadow / accumulate */
    float build_ms;             /* last art_scene_build, device time */
    float frame_ms;             /* last art_trace, device time (events on the context's stream) */
    float trace_primary_ms, shade_ms, trace_shadow_ms, accumulate_ms;
    float ao_ms;                /* last art_trace_ao (ray generation + any-hit + resolve) */
    uint32_t split_blocks;      /* fused frame: 8x8 pixel blocks the current wave plan deals to 4 or 16 waves instead of one (see ART_FLAG_FIXED_WAVES) */
    float refit_ms;             /* last refit after art_scene_set_model_matrix, device time (triangle records + every box above them) */
    float refit_cost_ratio;     /* surface-area cost of the refitted tree over the cost of the tree as built (the latest refit whose figure has arrived); 1 = as built */
    uint32_t refits, rebuilds;  /* refits since art_create; builds art_trace started by itself because refit_cost_ratio passed ArtTuning.refit_rebuild_ratio (include/art_parity.h; default 2) */
    float first_move_ms;        /* host time art_trace spent making the ring of structure versions at the first move of a built scene (0 with ART_FLAG_DYNAMIC_SCENE: art_scene_build made it, inside versions_ms) */
    float versions_ms;          /* host time of making that ring, wherever it was made */
} ArtStats;

typedef struct ArtContext ArtContext;

const char *art_last_error(void);
int32_t art_device_count(void);

/* VulkanTempleRayTracedRenderer::new (renderer.rs:140) / Drop */
int32_t art_create(const ArtConfig *cfg, ArtContext **out);
int32_t art_destroy(ArtContext *ctx);
/* use an externally owned hipStream_t (e.g. torch's current stream); NULL restores the context's own stream.
 * Only for one frame in flight: a ring owns its streams (art_stream_wait_frame / art_wait_external_event in include/art_parity.h hand frames over to other streams). */
int32_t art_set_stream(ArtContext *ctx, void *hip_stream);
/* Several frames per launch (1..4; default 1; the fused frame only): every art_trace then traces n frames with ONE launch -- frame b with
 * the camera cams[b] of art_set_camera_batch (art_set_camera sets all n alike) -- and a ring slot holds n frames: every per-slot output,
 * the compact tile buffer included (bind n x the single-frame size: frame b's tiles follow frame b - 1's), is n frames back to back, and
 * the unit of art_trace, ring slots, art_frames_in_flight and art_frames_done is a launch.  A launch costs ~7 us of machine time whatever
 * it traces, which a 1/8 share of a 1080p frame (21 us of tracing) feels: 27.6 -> 24.4 -> 22.5 us per frame at 1 / 2 / 4 frames per launch
 * (profiles/README.md r1o).  art_read_*, art_device_* and art_get_stats refer to frame art_set_read_frame selects (default 0) of the
 * latest launch; art_trace_ao and art_present are not available with n > 1.  Synchronises; bound tile buffers are unbound. */
int32_t art_set_frames_per_launch(ArtContext *ctx, uint32_t n);
int32_t art_set_camera_batch(ArtContext *ctx, const ArtCamera *cams, uint32_t n);
int32_t art_set_read_frame(ArtContext *ctx, uint32_t b);
/* frame ring: number of slots and the slot the NEXT art_trace will use */
int32_t art_frames_in_flight(ArtContext *ctx, uint32_t *frames, uint32_t *next_slot);
/* host-side, non-blocking: have frames [first, first + count) of this context (counted from 0 in art_trace order, at most 128 back) all
 * finished?  *traced (optional) receives the number of frames traced so far.  An exchange that is SUBMITTED only once its frames are done
 * needs no device-side wait per frame: on a GPU that keeps tracing, every hipStreamWaitEvent packet in the exchange stream took ~40 us to
 * retire, which capped a 1/7 share at 46 us per frame (profiles/README.md r1n). */
int32_t art_frames_done(ArtContext *ctx, uint64_t first, uint32_t count, int32_t *done, uint64_t *traced);
/* add_model (renderer.rs:346) -> VkModel::create_blas geometry contract (vk_model.rs:886-943): one call per glTF
 * primitive.  idx_bytes = 2|4 (vk_model.rs:142-150); rgba8 = 3 layers albedo/ORM/normal of tw x th texels
 * (model_reader.rs:14-19); model3x4 = row-major object->world (vk_model.rs:358-363).  Data are copied. */
int32_t art_scene_add_primitive(ArtContext *ctx, const ArtVertex *verts, uint32_t n_verts, const void *indices,
                                uint32_t n_indices, uint32_t idx_bytes, const uint8_t *rgba8, uint32_t tw, uint32_t th,
                                const float model3x4[12], uint32_t *out_primitive_id);
int32_t art_scene_clear(ArtContext *ctx);
/* residency (vk_model.rs:334-345, renderer.rs:637-651): only models in the Device state are instanced in the TLAS.  A disabled
 * primitive keeps its id and its host copy but is not traced.  A primitive that is part of the built structure leaves and re-enters it WITHOUT a build: the refit
 * in front of the next art_trace (see art_scene_set_model_matrix) writes its triangles nowhere / back and shrinks / grows every box above them -- frames are those
 * of a scene built without / with it, bit for bit; its device arrays stay until the next art_scene_build.  A primitive that was disabled when the scene was built
 * (never uploaded) needs art_scene_build to appear: art_scene_needs_build says which case the context is in. */
int32_t art_scene_set_primitive_enabled(ArtContext *ctx, uint32_t primitive_id, int32_t enabled);
/* Alpha-masked primitives (glTF alphaMode MASK; in Vulkan terms non-opaque geometry whose any-hit shader ignores the intersection when alpha < cutoff): a candidate
 * hit on primitive `primitive_id` is discarded when cutoff > 0 and the alpha of its texture layer 0 (byte 3, bilinear / REPEAT / LOD 0 at the hit's texture coordinate,
 * the sampler of the shading) is below cutoff -- for every ray: primary, shadow (a cut texel lets the light through), AO and both queries.  0 (the default) is opaque.
 * May be called at any time; on a built scene nothing is built: the NEXT art_trace (or query) takes it up, as for art_scene_set_primitive_enabled, and frames in flight
 * keep the cutoffs they were launched with.  NaN, a value outside [0, 1], an unknown id or a null context is ART_E_INVALID and changes nothing.  Scenes in which no
 * enabled primitive has a cutoff > 0 run the kernels without the test.  Every rank of an art_mgpu job must make the same calls.  DESIGN.md 3.2. */
int32_t art_scene_set_alpha_cutoff(ArtContext *ctx, uint32_t primitive_id, float cutoff);
/* Ray visibility masks (Vulkan: VkAccelerationStructureInstanceKHR.mask against traceRayEXT's cullMask; the reference hard-codes both to 0xFF, vk_model.rs:373,
 * raytrace.rgen.glsl:92,169): every primitive has an 8-bit visibility mask and every ray an 8-bit cull mask, 0xFF each by default.  A candidate hit on a primitive is
 * discarded iff (mask of the primitive & cull mask of the ray) == 0 -- per candidate, before the alpha test (an invisible candidate fetches no texel), for primary,
 * shadow and AO rays and the masked queries of art_parity.h.  The library gives the bits no meaning; the names below are a convention only. */
#define ART_MASK_ALL 255u /* 0xFF */
#define ART_VIS_CAMERA 1u
#define ART_VIS_SHADOW 2u
#define ART_VIS_AO 4u
#define ART_VIS_QUERY 8u
/* The visibility mask of primitive `primitive_id`.  May be called at any time; on a built scene nothing is built: the NEXT art_trace (or query) takes it up, as for
 * art_scene_set_alpha_cutoff, and frames in flight keep the masks they were launched with; a rebuild takes the masks along.  ArtStats.rebuilds and
 * art_scene_needs_build are untouched.  A mask above 0xFF, an unknown id or a null context is ART_E_INVALID and changes nothing.  Every rank of an art_mgpu job
 * must make the same calls.  DESIGN.md 3.4. */
int32_t art_scene_set_primitive_mask(ArtContext *ctx, uint32_t primitive_id, uint32_t mask);
/* The cull masks of the rays art_trace (primary, shadow) and art_trace_ao (ao) cast.  Per-launch state like the camera: a frame keeps what was current at its
 * art_trace -- art_trace_ao casts its rays with the AO mask of the frame it follows -- and all frames of a launch (art_set_frames_per_launch) share them.  0 is
 * legal: such a ray sees nothing.  A shadow ray is traced, and counted in ArtStats.shadow_rays, whether or not it can see anything; hit_pixels follows what the
 * primary rays see.  A value above 0xFF or a null context is ART_E_INVALID and changes nothing.  Scenes in which every enabled primitive has the mask 0xFF and no
 * cutoff, traced with no cull mask of 0, run the kernels without the test. */
int32_t art_set_ray_masks(ArtContext *ctx, uint32_t primary, uint32_t shadow, uint32_t ao);
/* 1: the next art_trace would fail with ART_E_STATE until art_scene_build has run (primitives added, or enabled that the last build did not contain); 0: it would not */
int32_t art_scene_needs_build(const ArtContext *ctx);
/* VkModel::set_model_matrix (vk_model.rs:461-466) -> get_transform_model_matrix (:358-363) -> the instance record of the per-frame TLAS
 * (VkTlasBuilder::recreate_tlas every frame, renderer.rs:637-651, vk_tlas_builder.rs:38-233): primitives first_primitive .. first_primitive + n_primitives - 1
 * (one model's, art_scene_add_glb returns the range) get a new row-major object->world 3x4.  On a built scene nothing is built again: the NEXT art_trace
 * (or query) first REFITS on the device -- the world-space triangle records and every node box above them, the topology kept -- on that frame's own stream,
 * into the next of a small ring of versions of the structure (4 by default; ArtTuning.as_versions in include/art_parity.h), so frames in flight keep the scene they were launched
 * with and nothing waits unless every version is still being read (the reference's per-frame fence, renderer.rs:451-466).  Frames are those of a fresh
 * build, bit for bit (hits are structure-independent).  When the refitted tree's surface-area cost passes ArtTuning.refit_rebuild_ratio (default 2) times
 * the built tree's, art_trace builds again instead (ArtStats.rebuilds).  Every rank of an art_mgpu job must make the same calls. */
int32_t art_scene_set_model_matrix(ArtContext *ctx, uint32_t first_primitive, uint32_t n_primitives, const float model3x4[12]);
/* BLAS update (vkCmdBuildAccelerationStructuresKHR, mode UPDATE, on a BLAS built with ALLOW_UPDATE -- the reference never
 * updates a BLAS: its flags are PREFER_FAST_TRACE only, vk_model.rs:968): primitive `primitive_id` gets n_verts new 48-byte
 * vertices (position, uv, normal, tangent: all of them), its indices, texture and model matrix kept.  n_verts must equal the
 * count it was added with.  Data are copied.  A null context or vertices, an unknown id or another count is ART_E_INVALID and
 * changes nothing; values are accepted as art_scene_add_primitive accepts them.  On a primitive of the built structure this is
 * a move (see art_scene_set_model_matrix): nothing is built, the NEXT art_trace (or query) refits first, on the same streams and
 * with the same waits, into the next version of the structure -- its shading records too, which every version keeps a copy of
 * from the first deformation on (that call synchronises once and allocates them: 144 B a triangle per version but the first,
 * ART_E_NOMEM from this call if they do not fit).  Frames are those of a fresh build with the vertices current at their launch,
 * bit for bit; moves and deformations between two frames make one refit, and the rebuild rule (ArtTuning.refit_rebuild_ratio)
 * builds over the new vertices.  A primitive that left the structure by residency shows its new shape when it is enabled again;
 * one the built structure does not hold (added since, or disabled at the build) with the next art_scene_build.  Every rank of an
 * art_mgpu job must make the same calls. */
int32_t art_scene_set_vertices(ArtContext *ctx, uint32_t primitive_id, const ArtVertex *verts, uint32_t n_verts);
/* art_scene_set_vertices with the data in DEVICE memory (GPU skinning, cloth, a physics step, a learned deformation in torch): no trip through the host.
 * MEANING: that of art_scene_set_vertices.  Frames, casts and queries called AFTER it are those of a fresh build over the new vertices, bit for bit; frames in
 * flight keep theirs; moves and deformations between two frames make one refit; the rebuild rule, residency, masks and cutoffs behave as for the host form.
 * LAYOUT: ART_VERTS_FULL replaces all 48 bytes of every vertex.  ART_VERTS_POSITIONS replaces the positions only -- three floats at verts_dev + i * stride_bytes for
 * vertex i -- and keeps uv, normal and tangent as they CURRENTLY are: as of the latest host-form or FULL call, or as added.  Shading normals therefore go stale under a
 * POSITIONS update; recomputing them is the caller's business.  Geometry (casts, crossings, nearest points, overlaps, depth) is exact.
 * STREAM ORDER: the library reads verts_dev ON hip_stream: the call enqueues one kernel there (behind whatever the caller enqueued earlier, such as the kernel that
 * produces the vertices) and returns.  Work enqueued on hip_stream afterwards may overwrite or free verts_dev; nothing else of the library ever reads it.  The refit in
 * front of the next art_trace or query waits for that kernel on the device, and the kernel for the refits that still read the primitive's previous vertices: nothing
 * waits on the host, and the steady state allocates nothing.  The first deformation of a built primitive in a context synchronises once and allocates the versions'
 * shading records, as for the host form (ART_E_NOMEM if they do not fit); no staging memory is allocated for a primitive only ever updated this way.
 * THE HOST COPY of the primitive falls behind; the library reads it back where it needs it (a build that lays the scene out again, art_scene_get_vertices).  A later
 * art_scene_set_vertices simply replaces it.  A POSITIONS call right after a host-form call first brings the device copy up to date, synchronously.
 * A primitive the built structure does not hold (added since the build, disabled at the build, no built scene) has no device copy: the call copies into the host
 * copy, synchronises hip_stream, and the vertices show with the next art_scene_build.
 * ERRORS change nothing and enqueue nothing: a null context, descriptor or verts_dev, an unknown id, another count, an unknown layout, a stride the layout does not
 * allow, verts_dev not 16-byte (FULL) or 4-byte (POSITIONS) aligned, flags or reserved other than 0 are ART_E_INVALID; ART_E_NO_DEVICE without a device.
 * Every rank of an art_mgpu job must make the same calls.  DESIGN.md 3.1. */
#define ART_VERTS_FULL 0u       /* n_verts x ArtVertex (48 B), all attributes replaced */
#define ART_VERTS_POSITIONS 1u  /* n_verts x 3 floats at stride_bytes: positions replaced, uv / normal / tangent kept as they are */
typedef struct ArtVertexUpdate {
    const void *verts_dev;   /* device memory (a torch tensor, any hipMalloc'ed memory) */
    void *hip_stream;        /* the stream verts_dev is produced on; NULL = a stream the context owns */
    uint32_t primitive_id;
    uint32_t n_verts;        /* must equal the count the primitive was added with */
    uint32_t layout;         /* ART_VERTS_* */
    uint32_t stride_bytes;   /* FULL: 0 or 48.  POSITIONS: 0 (= 12) or >= 12 and a multiple of 4 */
    uint32_t flags;          /* must be 0 */
    uint32_t reserved;       /* must be 0 */
} ArtVertexUpdate;           /* 40 bytes */
int32_t art_scene_set_vertices_device(ArtContext *ctx, const ArtVertexUpdate *u);
/* the primitive's current vertices (whichever form set them last), n_verts x 48 B into host memory; synchronises what it must (the latest device-form update of the
 * primitive, whose device copy is then read back).  A null context or dst, an unknown id or another count is ART_E_INVALID. */
int32_t art_scene_get_vertices(ArtContext *ctx, uint32_t primitive_id, ArtVertex *dst, uint32_t n_verts);
/* VkBlasBuilder::build_blas_from_geometry (vk_blas_builder.rs:88-170) + VkTlasBuilder::recreate_tlas
 * (vk_tlas_builder.rs:38-233): device LBVH over the world-space triangle soup. */
int32_t art_scene_build(ArtContext *ctx);

/* VkCamera::update_host_buffer (vk_camera.rs:104-126): the 268-byte block; and its producer.  A block holding a NaN or an infinity is ART_E_INVALID, and so
 * are parameters that have no finite matrices (a direction along the up axis (0, -1, 0) or of zero length, fovy 0, znear == zfar): the reference would
 * render NaN.  Rays that still come out non-finite (a finite but singular block) are misses, as in the oracle. */
int32_t art_set_camera(ArtContext *ctx, const ArtCamera *cam);
int32_t art_camera_from_params(const float pos[3], const float dir[3], float aspect, float fovy, float znear,
                               float zfar, ArtCamera *out);

/* VkLights::update_host_and_device_buffer (vk_lights.rs:81-139): n 80-byte records -- at most 1024 (the reference's list is a Vec behind an SSBO of n x 80 bytes, vk_lights.rs:89-91:
 * no bound but memory; libart carries the first 16 in the kernel arguments of every launch and the rest in a table per ring slot, so a frame in flight never sees a later list);
 * and their producers (lights.rs:144-159, :228-243, :281-296, :383-403).  art_read_shadow_bits (include/art_parity.h) reports the first 16 lights; ArtStats.shadow_rays counts all. */
int32_t art_set_lights(ArtContext *ctx, const ArtLight *lights, uint32_t n);
int32_t art_light_point(const float pos[3], const float color[3], float falloff, int32_t casts_shadows, ArtLight *out);
int32_t art_light_spot(const float pos[3], const float dir[3], const float color[3], float falloff, float penumbra,
                       float umbra, int32_t casts_shadows, ArtLight *out);
int32_t art_light_directional(const float dir[3], const float color[3], int32_t casts_shadows, ArtLight *out);
int32_t art_light_area(const float pos[3], const float pos2[3], const float pos3[3], int32_t invert_normal,
                       const float color[3], float falloff, float penumbra, float umbra, int32_t casts_shadows,
                       ArtLight *out);

/* VkRTLightningShadows::resize (vk_rt_lightning_shadows.rs:125-159) */
int32_t art_resize(ArtContext *ctx, uint32_t width, uint32_t height);
/* VkRTLightningShadows::trace_rays (vk_rt_lightning_shadows.rs:185-278): raygen + closest hit + light loop +
 * shadow rays + G-buffer stores of raytrace.rgen.glsl:77-200, asynchronous on the context's stream */
int32_t art_trace(ArtContext *ctx);
/* ray-traced ambient occlusion replacing VkXeGtao::compute_ao (vk_xe_gtao.rs:416-642) with the same I/O contract:
 * inputs = the depth + view-space normal outputs of the frame just traced (vk_xe_gtao.rs:295-333), output = one value
 * 0..255 per pixel in an R32_UINT-like buffer, as tonemap.comp.glsl:33-34 consumes it.  spp (1..64) cosine-weighted
 * any-hit rays of length `radius` per hit pixel (reference radius: 0.2 * 1.457, vk_xe_gtao.rs:17-18,:261), Hilbert-R2
 * noise (main_pass.comp.hlsl:48-65), final power 2.2 (vk_xe_gtao.rs:22).  Enqueued behind art_trace on its stream. */
int32_t art_trace_ao(ArtContext *ctx, uint32_t spp, float radius);
int32_t art_read_ao(ArtContext *ctx, void *dst, size_t bytes); /* width*height uint32 */
/* the step after the path (tonemap_layer.present, renderer.rs:566-615 / vk_tonemap.rs:469-552): packs the latest frame's
 * outputs as the reference stores them (colour + normal B10G11R11_UFLOAT_PACK32: renderer.rs:268, vk_rt_lightning_shadows.rs:152;
 * depth R16_SFLOAT: :142) and tonemaps like tonemap.comp.glsl:29-40 -- packed colour * ao/255 (255 if art_trace_ao has not run for
 * this frame) -> LpmFilter(LPM_CONFIG_709_709, control block of vk_tonemap.rs:417-426) -> pow(1/2.2) -> B8G8R8A8_UNORM. */
int32_t art_present(ArtContext *ctx);
int32_t art_read_present(ArtContext *ctx, void *dst_bgra8, size_t bytes);                       /* width*height*4 */
int32_t art_read_packed(ArtContext *ctx, void *color_b10g11r11, void *normal_b10g11r11, void *depth_f16); /* any may be NULL */
/* LpmData::new (vk_tonemap.rs:54-325): the 24 x uvec4 control block, host only */
int32_t art_lpm_control_block(int32_t shoulder, float soft_gap, float hdr_max, float exposure, float contrast, float shoulder_contrast,
                              const float saturation[3], const float crosstalk[3], uint32_t ctl[96]);
/* the fence (renderer.rs:451-466) */
int32_t art_sync(ArtContext *ctx);

/* ---- rays of the application's own (new functionality: in Vulkan terms traceRayEXT from a ray-generation shader the APPLICATION wrote, or VK_KHR_ray_query --
 * the reference has no call for it: its only rays are the pixels of raytrace.rgen.glsl and their shadow rays) -----------------------------------------------
 * One cast traces n rays that sit in a DEVICE buffer (a torch tensor, any hipMalloc'ed memory) through the built structure and leaves one record per ray in
 * device buffers, on a stream: lidar and sensor models, visibility and light probes, picking, collision rays, anything the caller shades itself.
 *  - Results: those of art_query_closest_masked / art_query_any_masked (include/art_parity.h, now host wrappers over the same path) for the same rays, bit for
 *    bit -- accept() and t_eff of DESIGN.md 1.1, the closest hit the argmin of (t_eff, global triangle id); u, v the barycentrics of vertices 1 and 2; ids the
 *    primitive id art_scene_add_primitive gave and the triangle's index in that primitive; a miss is (tmax, 0, 0, 0) and (-1, -1); a ray with a non-finite origin
 *    or direction or a NaN tmax is a miss; a candidate is first tested against the visibility masks (primitive's mask & cull_mask == 0: discarded, no texel
 *    fetched), then against its primitive's alpha cutoff.  A ray's record depends on that ray alone: the order of the rays in the buffer cannot matter.
 *  - Asynchronous: the call enqueues and returns.  It makes no hipMalloc / hipFree, synchronises with nothing and does not wait for frames in flight (the first
 *    cast of a context creates its cast stream, cursor blocks and events, and the first cast of a freshly built scene may complete the structure -- the 4-wide
 *    nodes, the ring of versions of a scene that moved -- as the first art_trace would).  The records are ordered behind the cast on hip_stream; with hip_stream
 *    NULL, on a stream the context owns for casts, whose fence is art_cast_sync.  Casts on one stream run in call order.  Casts and frames are unordered against
 *    each other and neither changes the other's results.
 *  - Scene: a cast sees the scene as of the call, like a frame: a pending move, deformation, residency switch, alpha cutoff or primitive mask is taken up first
 *    (the refit runs on a stream of the context in front of the cast; only events cross over to a caller's stream), and the cast holds the version of the
 *    structure it was launched on until it finishes: a refit that would rewrite that version waits for it on the host first, as it does for frames.
 *  - Host waits, counted by art_cast_counts: that wait, and the pool of per-cast work-cursor blocks running dry -- it is ART_CAST_POOL deep: the 33rd cast in
 *    flight waits for the oldest.  art_scene_build (the rebuild art_trace or a cast starts by itself included), art_set_tuning, art_resize, art_scene_clear,
 *    art_sync and art_destroy wait for outstanding casts.
 *  - Errors change nothing and enqueue nothing.  ART_E_INVALID: a null context or descriptor; a null, superfluous or misaligned pointer for the kind; an unknown
 *    kind; cull_mask above 0xFF; flags other than 0; n above ART_CAST_MAX_RAYS.  ART_E_STATE: the scene is not built, or art_scene_needs_build.  The output
 *    buffers must not overlap the rays: the caller's contract, not checked.
 *  - Sharded contexts and several frames per launch cast like any other: a cast depends on neither the extent nor the shard.  (Not through art_mgpu_*.) */
#define ART_CAST_CLOSEST 0u
#define ART_CAST_ANY 1u
/* the tracer's slot arithmetic is 32-bit: it hands out chunks of 64 .. 65536 rays, and n + the largest chunk (hence every chunk end, and 8 x the number of
 * chunks, which its per-XCD cursors are cut by) must fit -- 2^31 - 65536 */
#define ART_CAST_MAX_RAYS 2147418112u
#define ART_CAST_POOL 32u
typedef struct ArtRayCast {
    const void *rays_dev;  /* n x 8 floats: o.xyz, tmin, d.xyz, tmax (the layout of the queries); 16-byte aligned */
    void *tuv_dev;         /* CLOSEST: n x 4 floats t,u,v,0 -- a miss is (tmax,0,0,0); 16-byte aligned.  ANY: must be NULL */
    void *ids_dev;         /* CLOSEST: n x 2 int32 (primitive id as art_scene_add_primitive gave it, triangle in the primitive), -1,-1 for a miss; 8-byte aligned.  ANY: must be NULL */
    void *hit_dev;         /* ANY: n x uint8, 1 = something within [tmin, tmax].  CLOSEST: must be NULL */
    void *hip_stream;      /* hipStream_t the cast is enqueued on (e.g. torch's current stream); NULL = a stream the context owns for casts */
    uint32_t n;            /* 0 is legal: nothing is enqueued */
    uint32_t kind;         /* ART_CAST_* */
    uint32_t cull_mask;    /* 0..0xFF, as art_set_ray_masks; 0 sees nothing */
    uint32_t flags;        /* must be 0 */
} ArtRayCast;
int32_t art_cast_rays(ArtContext *ctx, const ArtRayCast *cast);
/* The first K hits along each ray, in order: what the ray goes through -- multi-return lidar, thickness and penetration, transparency the caller composites
 * itself.  In Vulkan terms an any-hit shader that records the intersection and calls ignoreIntersectionEXT, in one pass: no peeling, and hits that tie on t are all there.
 *  - Results: for a ray let A be the triangles accept() takes that the visibility masks do not discard (primitive's mask & cull_mask != 0; tested first) and
 *    the alpha cutoff does not cut.  Records 0 .. c-1 of the ray, c = min(|A|, max_hits), are the first c elements of A in ascending (t_eff, global triangle id), each the
 *    closest cast's record: (t_eff, u, v, 0) and (primitive id, triangle in the primitive).  Records c .. max_hits-1 are the miss record (tmax, 0, 0, 0), (-1, -1), and
 *    count_dev[i] = c.  A ray with a non-finite origin or direction or a NaN tmax has c = 0 and max_hits miss records that carry tmax as given.  With max_hits = 1 the
 *    records are those of ART_CAST_CLOSEST, bit for bit.  A ray's records depend on that ray alone.
 *  - Everything else is art_cast_rays's: asynchronous on hip_stream (NULL: the context's cast stream), the scene as of the call with the refit in front of the cast and the
 *    version held until the cast finishes, the same ring of ART_CAST_POOL cursor blocks and the same host waits; art_cast_counts counts it, art_cast_sync, art_sync,
 *    art_scene_build and the others wait for it.
 *  - Errors change nothing and enqueue nothing.  ART_E_INVALID: a null context or descriptor; a null or misaligned rays_dev / tuv_dev / ids_dev (with n = 0 a null buffer is
 *    one of no rays); max_hits 0 or above ART_CAST_MAX_HITS; cull_mask above 0xFF; flags other than 0; n above ART_CAST_MAX_RAYS.  ART_E_STATE: the scene is not built, or
 *    art_scene_needs_build.  The output buffers must not overlap the rays or each other: the caller's contract, not checked. */
#define ART_CAST_MAX_HITS 8u
typedef struct ArtRayCastMulti {
    const void *rays_dev;  /* n x 8 floats, as ArtRayCast; 16-byte aligned */
    void *tuv_dev;         /* n x max_hits x 4 floats, ray-major: ray i's record j at (i*max_hits + j); 16-byte aligned */
    void *ids_dev;         /* n x max_hits x 2 int32, same order; 8-byte aligned */
    void *count_dev;       /* n x uint8: records that are hits, 0..max_hits; may be NULL */
    void *hip_stream;      /* as ArtRayCast */
    uint32_t n;            /* 0 is legal: nothing is enqueued */
    uint32_t max_hits;     /* K: 1..ART_CAST_MAX_HITS */
    uint32_t cull_mask;    /* 0..0xFF */
    uint32_t flags;        /* must be 0 */
} ArtRayCastMulti;        /* 56 bytes */
int32_t art_cast_rays_multi(ArtContext *ctx, const ArtRayCastMulti *cast);
/* The surfaces each ray enters and leaves: how many triangles the ray crosses over its whole range, uncapped, and in which direction it crosses each --
 * what "is this point inside the mesh?", a signed distance, a solid voxelisation and a thickness count are made of.
 *  - Results: for a ray let A be art_cast_rays_multi's set: the triangles accept() takes (the triangle's own slab, then Moeller-Trumbore with
 *    tmin < t < tmax) that the visibility masks do not discard (primitive's mask & cull_mask != 0; tested first) and the alpha cutoff does not cut.  EVERY member of A is
 *    alpha-tested: every candidate counts, there is no "would win".  For a member of A let det = dot3(e1, cross3(d, e2)), d the ray's direction as given, e1 and e2 the
 *    triangle's world-space edges, dot3 and cross3 in their fmaf forms: the det Moeller-Trumbore itself forms (accept() has excluded det == 0).  The crossing is an
 *    ENTRY iff det > 0 and an EXIT iff det < 0: det = -d . (e1 x e2), so an entry goes against the winding normal ng of art_resolve_hits and an exit along it.
 *    Orientation is that of the world-space vertices: a mirroring model matrix swaps entries and exits, as it flips ng.  cross_dev[i] = (#entries, #exits), neither
 *    capped.  A ray with a non-finite origin or direction or a NaN tmax has (0, 0); tmax = +inf is legal.  A primitive that left the structure by residency is nowhere
 *    and is never counted.  A ray's record depends on that ray alone and on no property of the tree.
 *  - Exact, not topological: two triangles that share an edge BOTH accept a ray through that edge (the 1e-6 edge fattening of DESIGN.md 1.1 that makes closest hits
 *    watertight), so such a ray counts both.  A caller who wants inside / outside votes over several rays: the Python Renderer.points_inside does, with three.
 *  - Everything else is art_cast_rays's: asynchronous on hip_stream (NULL: the context's cast stream), the scene as of the call with the refit in front of the cast and the
 *    version held until the cast finishes, the same ring of ART_CAST_POOL cursor blocks and the same host waits; art_cast_counts counts it in casts and rays, art_cast_sync,
 *    art_sync, art_scene_build and the others wait for it.  (Not through art_mgpu_*.)
 *  - Errors change nothing and enqueue nothing.  ART_E_INVALID: a null context or descriptor; a null or misaligned rays_dev (16 bytes) or cross_dev (8 bytes) (with n = 0
 *    a null buffer is one of no rays); cull_mask above 0xFF; flags or reserved other than 0; n above ART_CAST_MAX_RAYS.  ART_E_STATE: the scene is not built, or
 *    art_scene_needs_build.  cross_dev must not overlap the rays: the caller's contract, not checked. */
typedef struct ArtRayCrossings {
    const void *rays_dev;  /* n x 8 floats o.xyz,tmin,d.xyz,tmax, as ArtRayCast; 16-byte aligned */
    void *cross_dev;       /* n x 2 uint32: (entries, exits); 8-byte aligned */
    void *hip_stream;      /* as ArtRayCast: NULL = the context's cast stream */
    uint32_t n;            /* 0 is legal: nothing is enqueued */
    uint32_t cull_mask;    /* 0..0xFF; 0 sees nothing */
    uint32_t flags;        /* must be 0 */
    uint32_t reserved;     /* must be 0 */
} ArtRayCrossings;         /* 40 bytes */
int32_t art_cast_crossings(ArtContext *ctx, const ArtRayCrossings *cast);
/* every cast enqueued so far has finished (those on callers' streams included) */
int32_t art_cast_sync(ArtContext *ctx);
/* since art_create: casts enqueued (n > 0), their rays, and the times art_cast_rays (or a refit in front of a frame) waited on the host for a cast.  Any pointer may be NULL. */
int32_t art_cast_counts(ArtContext *ctx, uint64_t *casts, uint64_t *rays, uint64_t *host_waits);
/* The surface behind hit records: what the ray hit.  Takes the (t,u,v) and (primitive, triangle) records art_cast_rays / art_cast_rays_multi write and
 * leaves, per record, the attributes the frame's own shading interpolates -- a G-buffer for the caller's rays: lidar intensity from the normal, compositing from alpha and
 * colour, picking and collision from the position.  No light, no shadow ray, no BRDF, no camera: a gather and an interpolation.
 *  - Values: those of the frame's surface block in its plain form (shade_surface_body<false>: no guarded fast path), same operations, same order.  Barycentrics (1-u-v, u, v)
 *    over the triangle's shading record; pos = object-to-world of the interpolated position; uv the interpolated texture coordinate (not wrapped); ns the frame's N
 *    (interpolated normal through world-to-object, tangent by Gram-Schmidt, binormal with vertex 0's handedness, texture layer 2, normalised); albedo and orm texture layers
 *    0 and 1 at uv through the frame's sampler (bilinear, REPEAT, LOD 0), raw: r,g,b,a in [0,1], no gamma -- albedo.a is the value the alpha cutoff tests.  ng =
 *    normalize(cross(w1 - w0, w2 - w0)) over the world-space vertices: orientation by winding, not flipped towards any ray; (0,0,0) where the cross product is zero.
 *  - The miss record is all zeros in every buffer given (pos.w = 0; a resolved record has pos.w = 1).  It is written for ids (-1,-1) and for every record that cannot be
 *    resolved safely: a primitive id outside [0, num_primitives), a triangle outside the primitive's, a primitive the built structure does not hold (added since the
 *    build, disabled at the build), a non-finite u or v.  The records are the caller's: all of it is checked before an address is formed -- a property of the kernel, not an
 *    error.  Finite u, v outside the triangle extrapolate.  A primitive that left the structure by residency (art_scene_set_primitive_enabled(.., 0) on a built one)
 *    still resolves: its shading records stay.  t is not read, and no rays are needed.  A record depends on its input record alone.  A NULL buffer is not written.
 *  - Scene and asynchrony: art_cast_rays's.  The scene as of the call (a pending move, deformation, residency switch or cutoff is taken up first, the refit on the context's
 *    streams in front of the resolve), the version current at the call held until the resolve finishes; enqueued on hip_stream (NULL: the context's cast stream) behind
 *    earlier work there -- a cast followed by a resolve of its buffers on one stream needs nothing in between -- without hipMalloc, hipFree or synchronisation on the steady
 *    path.  It takes a block of the casts' ring (ART_CAST_POOL): art_cast_sync, art_sync, art_scene_build and the others wait for it as for a cast, a refit that would
 *    rewrite the version it reads waits for it, and art_cast_counts' host_waits counts a wait it caused; casts and rays do not count it (it traces nothing).
 *  - Errors change nothing and enqueue nothing.  ART_E_INVALID: a null context or descriptor; a null or misaligned tuv_dev / ids_dev (with n = 0 null is fine); a misaligned
 *    output; all six outputs NULL with n > 0; flags other than 0; n above ART_CAST_MAX_RAYS.  ART_E_STATE: the scene is not built, or art_scene_needs_build.  Overlap
 *    between buffers is the caller's contract.  (Not through art_mgpu_*.) */
typedef struct ArtHitResolve {
    const void *tuv_dev;   /* n x 4 floats t,u,v,- : records as art_cast_rays / art_cast_rays_multi write them (for multi: n = rays x max_hits); 16-byte aligned */
    const void *ids_dev;   /* n x 2 int32 (primitive id, triangle in the primitive), -1,-1 = miss; 8-byte aligned */
    void *pos_dev;         /* n x float4: world position xyz; w = 1 for a resolved record, 0 for a miss record.  16-byte aligned.  May be NULL */
    void *ng_dev;          /* n x float4: geometric normal (unit, world space, orientation by winding: NOT flipped towards any ray), w = 0.  May be NULL */
    void *ns_dev;          /* n x float4: shading normal N (interpolated, TBN, normal map: the frame's N), w = 0.  May be NULL */
    void *uv_dev;          /* n x float2: interpolated texture coordinate (the frame's tu, tv; not wrapped); 8-byte aligned.  May be NULL */
    void *albedo_dev;      /* n x float4: texture layer 0 at uv as sample_tex returns it: r,g,b,a in [0,1], NO gamma (a is what the alpha cutoff tests).  May be NULL */
    void *orm_dev;         /* n x float4: texture layer 1 at uv, same sampler (y roughness, z metallic).  May be NULL */
    void *hip_stream;      /* as ArtRayCast: NULL = the context's cast stream */
    uint32_t n;            /* 0 is legal: nothing is enqueued */
    uint32_t flags;        /* must be 0 */
} ArtHitResolve;           /* 80 bytes */
int32_t art_resolve_hits(ArtContext *ctx, const ArtHitResolve *r);
/* The nearest surface point to a point (new functionality: Embree's rtcPointQuery -- the reference has no call for it, and no bundle of rays finds a
 * nearest point): collision and penetration depth, snapping, proximity and clearance, distance-field sampling, contact generation.  A query is (p.xyz, r): the nearest
 * point of the scene's triangles within distance r of p.
 *  - Results: defined exactly, like the casts', and independent of the structure.  For a triangle with global id g let d2_tri be the squared distance from p to it
 *    (DESIGN.md 3.8's formula: the face, then the three clamped edges, in fp32 without fused operations; a zero-area triangle is its segment or point), box_d2 the
 *    squared distance from p to the triangle's own box, d2_eff = max(d2_tri, box_d2).  The candidates are the triangles whose primitive's mask & cull_mask != 0 (tested
 *    first), with d2_tri and box_d2 finite and d2_eff <= r*r; the answer is the argmin over all of them of (d2_eff, g).  duv_dev[i] = (sqrtf(d2_eff), u, v, 0), u, v the
 *    barycentrics of vertices 1 and 2 of the nearest point (u, v >= 0, u + v <= 1 up to one rounding: a record art_resolve_hits takes); ids_dev[i] = (primitive id,
 *    triangle in the primitive) as a closest cast's; point_dev[i] (optional) = (v0 + (u*e1 + v*e2), 1).  A miss -- nothing within r -- is (r as given, 0, 0, 0), (-1, -1)
 *    and a point of zeros.  A query with a non-finite p, a NaN r or r < 0 is a miss; r = +inf is legal (a primitive that left the structure by residency is nowhere and
 *    is never returned), and so is -0.0.  A record depends on its query alone.
 *  - Alpha cutoffs are NOT tested: there is no ray to let through, and a triangle whose nearest point is cut would not have its nearest uncut point found.  Visibility
 *    masks apply as for casts: cull_mask 0 sees nothing.
 *  - Asynchrony and scene: art_cast_rays's.  The call enqueues on hip_stream (NULL: the context's cast stream) and returns: no hipMalloc / hipFree and no synchronisation
 *    on the steady path.  The scene as of the call -- a pending move, deformation, residency switch or primitive mask is taken up first, the refit in front of the
 *    queries -- and the version held until they finish.  It takes a block of the casts' ring (ART_CAST_POOL): art_cast_sync, art_sync, art_scene_build and the others
 *    wait for it as for a cast, and art_cast_counts' host_waits counts a wait it caused; casts and rays do not count it (it traces no ray).
 *  - Errors change nothing and enqueue nothing.  ART_E_INVALID: a null context or descriptor; a null or misaligned points_dev / duv_dev (16 bytes) / ids_dev (8 bytes) --
 *    with n = 0 null is fine; a misaligned point_dev; cull_mask above 0xFF; flags or reserved other than 0; n above ART_CAST_MAX_RAYS.  ART_E_STATE: the scene is not
 *    built, or art_scene_needs_build.  Overlap between buffers is the caller's contract.  (Not through art_mgpu_*.) */
typedef struct ArtPointQuery {
    const void *points_dev; /* n x 4 floats p.xyz, r; 16-byte aligned */
    void *duv_dev;          /* n x 4 floats d,u,v,0 -- a miss is (r,0,0,0); 16-byte aligned */
    void *ids_dev;          /* n x 2 int32 (primitive id, triangle in the primitive), -1,-1 for a miss; 8-byte aligned */
    void *point_dev;        /* n x float4: the nearest point xyz, w = 1; a miss is all zeros.  16-byte aligned.  May be NULL */
    void *hip_stream;       /* as ArtRayCast: NULL = the context's cast stream */
    uint32_t n;             /* 0 is legal: nothing is enqueued */
    uint32_t cull_mask;     /* 0..0xFF; 0 sees nothing */
    uint32_t flags;         /* must be 0 */
    uint32_t reserved;      /* must be 0 */
} ArtPointQuery;            /* 56 bytes */
int32_t art_closest_points(ArtContext *ctx, const ArtPointQuery *q);
/* A ball along a ray (new functionality: PhysX's sweep, Unity's SphereCast -- the reference has no call for it, a ray misses what the ball clips with
 * its side, and art_closest_points answers only where the ball stands): character and robot-link motion, drone and probe clearance along a path, continuous collision
 * of a thrown object, a lidar beam of finite width as a conservative tube.  A query is a ray of the casts' layout (o.xyz, tmin, d.xyz, tmax) and ONE radius for the
 * whole call: the ball's centre is c(t) = o + t*d (d need not be unit), and the answer is where the ball first touches the scene's triangles with tmin <= t < tmax.
 *  - Results: defined exactly, like the casts', and independent of the structure.  For a triangle with global id g, t_tri is the smallest t among the taken features --
 *    the ball overlaps the triangle at tmin already (S), its centre reaches the plane at distance radius above the face (F), the cylinder round an edge (E01, E02, E12:
 *    the entry root, the edge's direction projected out first) or the sphere round a vertex (V0, V1, V2), DESIGN.md 3.9's formulas in that order, fp32 without fused
 *    operations, the first of equals; tn the entry of section 1.1's slab into the triangle's own box inflated by the radius; t_eff = max(t_tri, tn).  The candidates
 *    are the triangles whose primitive's mask & cull_mask != 0 (tested first), with some feature taken and the slab passed; the answer is the argmin over all of
 *    them of (t_eff, g).  tuv_dev[i] = (t_eff, u, v, 0), u, v the barycentrics of vertices 1 and 2 of the contact point (a record art_resolve_hits takes); ids_dev[i]
 *    as a closest cast's; point_dev[i] (optional) = (v0 + (u*e1 + v*e2), 1): the contact normal is normalize(c(t) - point).  A miss is (tmax as given, 0, 0, 0),
 *    (-1, -1) and a point of zeros.  A ray with a non-finite o or d or a NaN tmax is a miss.  d = 0 is legal: a ball that does not move, only S answers.  radius = 0
 *    is legal: a thin ray BY THIS FORMULA, not bit-equal to ART_CAST_CLOSEST (no fattened edges, other operations).  A record depends on its ray and the radius alone.
 *  - Alpha cutoffs are NOT tested, for art_closest_points' reason.  Visibility masks apply as for casts: cull_mask 0 sees nothing.  A primitive that left the
 *    structure by residency is nowhere and is never returned.
 *  - Asynchrony and scene: art_cast_rays's, with no path of its own -- stream, no allocation or synchronisation on the steady path, the scene as of the call, the
 *    version held, a block of the casts' ring (ART_CAST_POOL), the same fences.  It traces rays: art_cast_counts counts it in casts and rays.
 *  - Errors change nothing and enqueue nothing.  ART_E_INVALID: a null context or descriptor; a null or misaligned rays_dev / tuv_dev (16 bytes) / ids_dev (8 bytes) --
 *    with n = 0 null is fine; a misaligned point_dev; a radius that is NaN, negative (-0.0 is 0) or infinite; cull_mask above 0xFF; flags other than 0; n above
 *    ART_CAST_MAX_RAYS.  ART_E_STATE: the scene is not built, or art_scene_needs_build.  Overlap between buffers is the caller's contract.  (Not through art_mgpu_*.) */
typedef struct ArtSphereCast {
    const void *rays_dev;   /* n x 8 floats o.xyz,tmin,d.xyz,tmax; 16-byte aligned */
    void *tuv_dev;          /* n x 4 floats t,u,v,0 -- a miss is (tmax,0,0,0); 16-byte aligned */
    void *ids_dev;          /* n x 2 int32 (primitive id, triangle in the primitive), -1,-1 for a miss; 8-byte aligned */
    void *point_dev;        /* n x float4: the contact point xyz, w = 1; a miss is all zeros.  16-byte aligned.  May be NULL */
    void *hip_stream;       /* as ArtRayCast: NULL = the context's cast stream */
    uint32_t n;             /* 0 is legal: nothing is enqueued */
    uint32_t cull_mask;     /* 0..0xFF; 0 sees nothing */
    uint32_t flags;         /* must be 0 */
    float radius;           /* of the ball, for every ray of the call: finite, >= 0 */
} ArtSphereCast;            /* 56 bytes */
int32_t art_cast_spheres(ArtContext *ctx, const ArtSphereCast *s);
/* The K nearest triangles to a point (new functionality: an rtcPointQuery callback that collects instead of shrinking, PhysX's overlap that reports what
 * it touches): every face a ball rests on for a contact manifold, the clearance against the second-nearest wall, neighbours for a distance field, snapping that chooses
 * among candidates.  A query is art_closest_points' (p.xyz, r); the answer is up to max_hits records a query.
 *  - Results: defined exactly and independent of the structure, with art_closest_points' formulas unchanged (d2_tri, box_d2, d2_eff = max of the two, the point).  Let A
 *    be the query's candidates there: the triangles whose primitive's mask & cull_mask != 0 (tested first), with d2_tri and box_d2 finite and d2_eff <= r*r.  Records
 *    0 .. c-1 of the query, c = min(|A|, max_hits), are the first c elements of A in ascending (d2_eff, global triangle id), each art_closest_points' own record for
 *    that triangle: duv (sqrtf(d2_eff), u, v, 0), ids (primitive id, triangle in the primitive), point (v0 + (u*e1 + v*e2), 1).  Records c .. max_hits-1 are the miss
 *    record -- (r as given, 0, 0, 0), (-1, -1), a point of zeros -- and count_dev[i] = c.  The answers are the K nearest TRIANGLES, not K distinct points: the triangles
 *    that share the nearest edge or vertex all appear, at the same distance and with the same point, ordered by global id.  Every record is one art_resolve_hits takes
 *    (n x max_hits of them, flattened).  With max_hits = 1 the records are art_closest_points', bit for bit.  A query's records depend on that query alone.
 *  - A query with a non-finite p, a NaN r or r < 0 has c = 0 and max_hits miss records that carry r as given; r = +inf and -0.0 are legal.  Alpha cutoffs are NOT
 *    tested, for art_closest_points' reason; visibility masks apply as for casts (cull_mask 0 sees nothing); a primitive that left the structure by residency is nowhere
 *    and is never returned.
 *  - Asynchrony and scene: art_closest_points', with no path of its own -- stream, no allocation or synchronisation on the steady path, the scene as of the call, the
 *    version held, a block of the casts' ring (ART_CAST_POOL), the same fences.  art_cast_counts counts it in neither casts nor rays (it traces no ray); a host wait it
 *    causes counts in host_waits.
 *  - Errors change nothing and enqueue nothing.  ART_E_INVALID: a null context or descriptor; a null or misaligned points_dev / duv_dev (16 bytes) / ids_dev (8 bytes) --
 *    with n = 0 null is fine; a misaligned point_dev; max_hits 0 or above ART_CAST_MAX_HITS; cull_mask above 0xFF; flags other than 0; n above ART_CAST_MAX_RAYS.
 *    ART_E_STATE: the scene is not built, or art_scene_needs_build.  Overlap between buffers is the caller's contract.  (Not through art_mgpu_*.) */
typedef struct ArtPointQueryMulti {
    const void *points_dev; /* n x 4 floats p.xyz, r; 16-byte aligned (ArtPointQuery's) */
    void *duv_dev;          /* n x max_hits x 4 floats d,u,v,0, query-major: query i's record j at i*max_hits + j; 16-byte aligned */
    void *ids_dev;          /* n x max_hits x 2 int32, same order; 8-byte aligned */
    void *point_dev;        /* n x max_hits x float4, same order; 16-byte aligned.  May be NULL */
    void *count_dev;        /* n x uint8: records that are answers, 0..max_hits.  May be NULL */
    void *hip_stream;       /* as ArtRayCast */
    uint32_t n;             /* 0 is legal: nothing is enqueued */
    uint32_t max_hits;      /* K: 1..ART_CAST_MAX_HITS */
    uint32_t cull_mask;     /* 0..0xFF */
    uint32_t flags;         /* must be 0 */
} ArtPointQueryMulti;       /* 64 bytes */
int32_t art_closest_points_multi(ArtContext *ctx, const ArtPointQueryMulti *q);
/* The triangles that touch a box (new functionality: PhysX's overlap with a box geometry, Unity's OverlapBox / CheckBox -- the reference has no call
 * for it): an occupancy grid of the scene (a voxelisation, which rays parallel to a surface miss and a ball round the cell overstates), trigger volumes, broad-phase
 * candidates for a box-shaped body, the triangles of a region for a baker or a learned model.  A query is a closed world-axis box [lo, hi].
 *  - Results: defined exactly and independent of the structure.  A triangle with global id g and record v0, e1, e2, tlo, thi (its own box) OVERLAPS the box iff (1) tlo.x <
 *    3.0e38 (a primitive that left the structure by residency is nowhere and is never returned); (2) the boxes meet: on every axis tlo <= hi and lo <= thi, comparisons
 *    only; (3) the triangle's plane does not separate and (4) none of the nine axes e_k x f_j does -- Akenine-Moeller's test about c = 0.5*lo + 0.5*hi with h = 0.5*hi -
 *    0.5*lo, DESIGN.md 3.11's formulas in fp32 without fused operations, sums of three as (a + b) + c; a comparison with a NaN is false, so such an axis separates nothing;
 *    a zero-area triangle goes through the same formulas.  Touching counts: a triangle in the face two boxes share belongs to both.  The candidates are the overlapping
 *    triangles whose primitive's mask & cull_mask != 0 (cull_mask 0 sees nothing); alpha cutoffs are NOT tested, for art_closest_points' reason.
 *  - ART_OVERLAP_ANY: hit_dev[i] = 1 iff the box has a candidate, else 0; the walk ends at the first one.  ART_OVERLAP_LIST: count_dev[i] (optional) = the number of
 *    candidates, all of them, not capped by max_hits; records 0 .. c-1 of the box, c = min(count, max_hits), are (primitive id, triangle in the primitive) of the
 *    candidates in ascending g; records c .. max_hits-1 are (-1, -1).  A box with a non-finite coordinate or with lo > hi on any axis is dead: hit 0, count 0, miss
 *    records, no walk.  lo == hi is legal (a point, a segment, a rectangle).  Words 3 and 7 of a box are not read.  A box's answer depends on that box alone.
 *  - Asynchrony and scene: art_closest_points', with no path of its own -- stream, no allocation or synchronisation on the steady path, the scene as of the call, the
 *    version held, a block of the casts' ring (ART_CAST_POOL), the same fences.  art_cast_counts counts it in neither casts nor rays (it traces no ray); a host wait it
 *    causes counts in host_waits.
 *  - Errors change nothing and enqueue nothing.  ART_E_INVALID: a null context or descriptor; flags or reserved other than 0; a kind that is neither; cull_mask above
 *    0xFF; n above ART_CAST_MAX_RAYS; a null or misaligned boxes_dev (16 bytes; with n = 0 null is fine); ANY: ids_dev or count_dev given, max_hits other than 0, a null
 *    hit_dev; LIST: hit_dev given, max_hits 0 or above ART_CAST_MAX_HITS, a null or misaligned ids_dev (8 bytes), a misaligned count_dev (4 bytes).  ART_E_STATE: the
 *    scene is not built, or art_scene_needs_build.  Overlap between buffers is the caller's contract.  (Not through art_mgpu_*.) */
#define ART_OVERLAP_ANY 0u
#define ART_OVERLAP_LIST 1u
typedef struct ArtBoxQuery {
    const void *boxes_dev;  /* n x 8 floats: lo.xyz, -, hi.xyz, - (words 3 and 7 are not read); 16-byte aligned */
    void *hit_dev;          /* ANY: n x uint8, 1 = some triangle overlaps the box.  LIST: must be NULL */
    void *ids_dev;          /* LIST: n x max_hits x 2 int32 (primitive id, triangle in the primitive), box-major: box i's record j at i*max_hits + j; 8-byte aligned.  ANY: must be NULL */
    void *count_dev;        /* LIST: n x uint32: ALL overlapping triangles of the box, not capped by max_hits; 4-byte aligned.  May be NULL.  ANY: must be NULL */
    void *hip_stream;       /* as ArtRayCast */
    uint32_t n;             /* 0 is legal: nothing is enqueued */
    uint32_t kind;          /* ART_OVERLAP_ANY | ART_OVERLAP_LIST */
    uint32_t max_hits;      /* LIST: K, 1..ART_CAST_MAX_HITS.  ANY: must be 0 */
    uint32_t cull_mask;     /* 0..0xFF; 0 sees nothing */
    uint32_t flags;         /* must be 0 */
    uint32_t reserved;      /* must be 0 */
} ArtBoxQuery;              /* 64 bytes */
int32_t art_overlap_boxes(ArtContext *ctx, const ArtBoxQuery *q);
/* The scene triangles that touch query triangles (which is the definition; new functionality: Embree's rtcCollide, PhysX's overlap with a triangle-mesh
 * geometry, FCL's mesh-mesh test -- the reference has no call for it): does this mesh, where it now stands, cut the scene's surfaces, and which triangles does it cut --
 * a robot link, a tool, a vehicle hull, a character's proxy; an oriented box is twelve triangles of this query.  A query is a triangle q0, q1, q2.
 *  - Results: defined exactly and independent of the structure.  A triangle with global id g and record v0, e1, e2, tlo, thi (its own box) OVERLAPS the query iff (1) tlo.x <
 *    3.0e38 (a primitive that left the structure by residency is nowhere and is never returned); (2) the boxes meet: with qlo, qhi the componentwise minimum and maximum
 *    of the three vertices (two selects from the first), on every axis tlo <= qhi and qlo <= thi, comparisons only; (3) none of 17 axes separates: with a_m = q_m - v0,
 *    f = (e1, e2 - e1, -e2), g = (a1 - a0, a2 - a1, a0 - a2), n = cross(e1, e2), m = cross(g0, g1), the axes are n, m, the nine cross(f_i, g_j), the three cross(n, f_i)
 *    and the three cross(m, g_j); an axis x separates iff min(0, x.e1, x.e2) > max(x.a0, x.a1, x.a2) or max(0, x.e1, x.e2) < min(x.a0, x.a1, x.a2) -- DESIGN.md 3.13's
 *    formulas in fp32 without fused operations, sums of three as (a + b) + c, minima and maxima by selects; a comparison with a NaN is false, so a zero axis or one
 *    with a NaN separates nothing.  Every test is closed: touching counts, also at a single vertex.  Coplanar disjoint triangles are apart (the six in-plane axes).
 *    Zero-area scene triangles and zero-area queries (a segment, a point) go through the same formulas: for a zero-area operand lying in the other's plane that can be
 *    an overlap geometry would not call one.  The candidates are the overlapping triangles whose primitive's mask & cull_mask != 0 (cull_mask 0 sees nothing); alpha
 *    cutoffs are NOT tested, for art_closest_points' reason.
 *  - This is a SURFACE test: a query wholly inside a closed mesh touches nothing (Renderer.points_inside on one vertex answers containment).  Pruning is exact for
 *    art_overlap_boxes' reason: a child is skipped only when its decoded box misses [qlo, qhi] by comparison, or its byte box is inverted.
 *  - ART_OVERLAP_ANY: hit_dev[i] = 1 iff the query has a candidate, else 0; the walk ends at the first one.  ART_OVERLAP_LIST: count_dev[i] (optional) = the number of
 *    candidates, all of them, not capped by max_hits; records 0 .. c-1 of the query, c = min(count, max_hits), are (primitive id, triangle in the primitive) of the
 *    candidates in ascending g; records c .. max_hits-1 are (-1, -1).  A query with a non-finite coordinate among its nine is dead: hit 0, count 0, miss records, no
 *    walk.  Words 3, 7 and 11 of a query are not read.  A query's answer depends on that query alone.
 *  - Asynchrony and scene: art_overlap_boxes', with no path of its own -- stream, no allocation or synchronisation on the steady path, the scene as of the call, the
 *    version held, a block of the casts' ring (ART_CAST_POOL), the same fences.  art_cast_counts counts it in neither casts nor rays (it traces no ray); a host wait it
 *    causes counts in host_waits.
 *  - Errors change nothing and enqueue nothing.  ART_E_INVALID: a null context or descriptor; flags or reserved other than 0; a kind that is neither; cull_mask above
 *    0xFF; n above ART_CAST_MAX_RAYS; a null or misaligned tris_dev (16 bytes; with n = 0 null is fine); ANY: ids_dev or count_dev given, max_hits other than 0, a null
 *    hit_dev; LIST: hit_dev given, max_hits 0 or above ART_CAST_MAX_HITS, a null or misaligned ids_dev (8 bytes), a misaligned count_dev (4 bytes).  ART_E_STATE: the
 *    scene is not built, or art_scene_needs_build.  Overlap between buffers is the caller's contract.  (Not through art_mgpu_*.) */
typedef struct ArtTriQuery {
    const void *tris_dev;   /* n x 12 floats: q0.xyz, -, q1.xyz, -, q2.xyz, - (words 3, 7 and 11 are not read); 16-byte aligned */
    void *hit_dev;          /* ANY: n x uint8, 1 = some triangle overlaps the query.  LIST: must be NULL */
    void *ids_dev;          /* LIST: n x max_hits x 2 int32 (primitive id, triangle in the primitive), query-major: query i's record j at i*max_hits + j; 8-byte aligned.  ANY: must be NULL */
    void *count_dev;        /* LIST: n x uint32: ALL candidates of the query, not capped by max_hits; 4-byte aligned.  May be NULL.  ANY: must be NULL */
    void *hip_stream;       /* as ArtRayCast */
    uint32_t n;             /* 0 is legal: nothing is enqueued */
    uint32_t kind;          /* ART_OVERLAP_ANY | ART_OVERLAP_LIST */
    uint32_t max_hits;      /* LIST: K, 1..ART_CAST_MAX_HITS.  ANY: must be 0 */
    uint32_t cull_mask;     /* 0..0xFF; 0 sees nothing */
    uint32_t flags;         /* must be 0 */
    uint32_t reserved;      /* must be 0 */
} ArtTriQuery;              /* 64 bytes */
int32_t art_overlap_triangles(ArtContext *ctx, const ArtTriQuery *q);
/* The distance from query triangles to the scene, and where (which is the definition; new functionality: FCL's distance, PhysX's computeDistance, PQP's
 * TriDist -- the reference has no call for it): the clearance of a mesh that art_overlap_triangles says cuts nothing -- a robot link 2 mm from a wall and one 2 m from it
 * -- which bundles of art_closest_points on sampled points miss where two edges cross.  A query is a triangle q0, q1, q2 and a search radius r in word 3.
 *  - Results: defined exactly and independent of the structure, in fp32 without fused operations, sums of three as (a + b) + c, minima and maxima by selects, every divisor
 *    guarded.  For a triangle with global id g and record v0, e1, e2, tlo, thi, with g1 = q1 - q0, g2 = q2 - q0: the FEATURES are, in this order, the first of the smallest
 *    winning, art_closest_points' d2_tri of q0, q1, q2 against the triangle; of v0, v0 + e1, v0 + e2 against the query (q0, g1, g2); and the nine pairs of scene edge
 *    (v0,e1), (v0,e2), (v0+e1,e2-e1) against query edge (q0,g1), (q0,g2), (q0+g1,g2-g1), scene edge outermost, by DESIGN.md 3.14's clamped segment formula.  d2_tri = 0 if
 *    art_overlap_triangles' condition 3 (the 17 axes) says the two touch or cut, else the winning feature's distance (+inf, the axes not asked, where no feature gives a
 *    number: a non-finite triangle); box_d2 = the squared distance between the query's box [qlo, qhi] and [tlo, thi]; d2_eff = max(d2_tri, box_d2).  The candidates are the
 *    triangles with tlo.x < 3.0e38 (a primitive that left the structure by residency is nowhere), whose primitive's mask & cull_mask != 0, with d2_tri and box_d2 finite
 *    and d2_eff <= r*r; the answer is the argmin of (d2_eff, g).  duv_dev[i] = (sqrtf(d2_eff), u, v, 0), u, v the barycentrics of vertices 1 and 2 of the witness point on
 *    the scene triangle (a record art_resolve_hits takes); ids_dev[i] as a closest cast's; point_dev[i] (optional) = (v0 + (u*e1 + v*e2), 1); qpoint_dev[i] (optional) =
 *    (q0 + (s*g1 + t*g2), 1), the witness on the query.  The witnesses are the winning feature's in both cases: for a cutting pair the two points are NOT a point of the
 *    intersection and need not coincide -- art_overlap_triangles says which triangles cut, this query says the clearance is 0.  Zero-area operands (a segment, a point) go
 *    through the same formulas.
 *  - A miss -- nothing within r -- is (r as given, 0, 0, 0), (-1, -1) and points of zeros.  A query with a non-finite coordinate among its nine, a NaN r or r < 0 is dead:
 *    its miss record, no walk.  r = +inf and -0.0 are legal.  Words 7 and 11 of a query are not read.  A record depends on its query alone.
 *  - Alpha cutoffs are NOT tested, for art_closest_points' reason.  Visibility masks apply as for casts: cull_mask 0 sees nothing.  Penetration depth is not computed.
 *  - Asynchrony and scene: art_closest_points', with no path of its own -- stream, no allocation or synchronisation on the steady path, the scene as of the call, the
 *    version held, a block of the casts' ring (ART_CAST_POOL), the same fences.  art_cast_counts counts it in neither casts nor rays (it traces no ray); a host wait it
 *    causes counts in host_waits.
 *  - Errors change nothing and enqueue nothing.  ART_E_INVALID: a null context or descriptor; flags or reserved other than 0; cull_mask above 0xFF; n above
 *    ART_CAST_MAX_RAYS; a null or misaligned tris_dev / duv_dev (16 bytes) / ids_dev (8 bytes) -- with n = 0 null is fine; a misaligned point_dev or qpoint_dev.
 *    ART_E_STATE: the scene is not built, or art_scene_needs_build.  Overlap between buffers is the caller's contract.  (Not through art_mgpu_*.) */
typedef struct ArtTriDistance {
    const void *tris_dev;   /* n x 12 floats: q0.xyz, r | q1.xyz, - | q2.xyz, - ; 16-byte aligned.  Word 3 is the query's radius; words 7 and 11 are not read */
    void *duv_dev;          /* n x 4 floats d,u,v,0 -- a miss is (r as given,0,0,0); 16-byte aligned */
    void *ids_dev;          /* n x 2 int32 (primitive id, triangle in the primitive), -1,-1 for a miss; 8-byte aligned */
    void *point_dev;        /* n x float4: the witness point on the SCENE triangle, w = 1; a miss is zeros.  16-byte aligned.  May be NULL */
    void *qpoint_dev;       /* n x float4: the witness point on the QUERY triangle, w = 1; a miss is zeros.  16-byte aligned.  May be NULL */
    void *hip_stream;       /* as ArtRayCast: NULL = the context's cast stream */
    uint32_t n, cull_mask, flags, reserved;   /* n = 0 is legal: nothing is enqueued; cull_mask 0..0xFF; flags, reserved: must be 0 */
} ArtTriDistance;           /* 64 bytes */
int32_t art_closest_triangles(ArtContext *ctx, const ArtTriDistance *q);
/* The first contact of translating query triangles with the scene (which is the definition; new functionality: PhysX's sweep with a mesh geometry,
 * Bullet's convex sweep, FCL's continuous collision -- the reference has no call for it): how far a body of triangles can move along a displacement before it touches the
 * scene, and where.  A query is 16 floats: q0.xyz, tmin | q1.xyz, tmax | q2.xyz, - | d.xyz, -.  The query triangle at time t is q_m + t*d (d need not be unit); the
 * answer is the first t with tmin <= t < tmax at which it touches a scene triangle.
 *  - Results: defined exactly and independent of the structure, in fp32 with nothing fused, sums of three as (a + b) + c, minima and maxima by selects, every divisor
 *    guarded.  For a triangle with global id g and record v0, e1, e2, tlo, thi, with g1 = q1 - q0, g2 = q2 - q0, the FEATURES are, in this order, the first of the
 *    smallest t in [tmin, tmax) winning: S, the start -- art_overlap_triangles' condition 3 holds for the query posed at tmin (q_m + tmin*d), t = tmin, witnesses
 *    art_closest_triangles' of that pose; each query vertex against the scene face and each scene vertex against the query face (the plane's t, then art_cast_spheres'
 *    face barycentrics, closed); the nine pairs of scene edge (v0,e1), (v0,e2), (v0+e1,e2-e1) and query edge (q0,g1), (q0,g2), (q0+g1,g2-g1), scene edge outermost
 *    (the t at which the two lines meet, both parameters in [0, 1]).  DESIGN.md 3.15 has every formula.  t_eff = fmaxf(t_tri, tn), tn the entry of the ray (0, d) into
 *    the box [tlo - qhi, thi - qlo] by art_cast_rays' slab with tmax for its limit ([qlo, qhi]: the box of the three vertices).  The candidates are the triangles with
 *    tlo.x < 3.0e38 (residency), whose primitive's mask & cull_mask != 0, with t_tri < inf, whose slab passes; the answer is the argmin of (t_eff, g).
 *    tuv_dev[i] = (t_eff, u, v, 0), u, v on the scene triangle (a record art_resolve_hits takes); ids_dev[i] as a closest cast's; point_dev[i] (optional) =
 *    (v0 + (u*e1 + v*e2), 1); qpoint_dev[i] (optional) = (q0 + (s*g1 + t*g2), 1), the witness on the query in its REST pose: add t_eff*d for the contact.
 *  - A miss is (tmax as given, 0, 0, 0), (-1, -1) and points of zeros.  A query with a non-finite value among its nine coordinates or in d, or a NaN tmax, is dead: its
 *    miss record, no walk.  d = 0 is legal: only S can answer.  Words 11 and 15 of a query are not read.  A record depends on its query alone.
 *  - LIMITATION: two coplanar triangles that slide within their common plane have a zero denominator in every moving feature; S alone sees them, so a contact that
 *    begins after tmin in that configuration is not reported.  Zero-area operands (a segment, a point) go through the same formulas.  No rotation during the sweep.
 *  - Alpha cutoffs are NOT tested, for art_closest_points' reason.  Visibility masks apply as for casts: cull_mask 0 sees nothing.
 *  - Asynchrony and scene: art_cast_rays', with no path of its own -- stream, no allocation or synchronisation on the steady path, the scene as of the call, the
 *    version held, a block of the casts' ring (ART_CAST_POOL), the same fences.  art_cast_counts counts it in casts and rays.
 *  - Errors change nothing and enqueue nothing.  ART_E_INVALID: a null context or descriptor; flags or reserved other than 0; cull_mask above 0xFF; n above
 *    ART_CAST_MAX_RAYS; a null or misaligned sweeps_dev / tuv_dev (16 bytes) / ids_dev (8 bytes) -- with n = 0 null is fine; a misaligned point_dev or qpoint_dev.
 *    ART_E_STATE: the scene is not built, or art_scene_needs_build.  Overlap between buffers is the caller's contract.  (Not through art_mgpu_*.) */
typedef struct ArtTriCast {
    const void *sweeps_dev; /* n x 16 floats: q0.xyz, tmin | q1.xyz, tmax | q2.xyz, - | d.xyz, - ; 16-byte aligned.  Words 11 and 15 are not read */
    void *tuv_dev;          /* n x 4 floats t,u,v,0 -- a miss is (tmax as given,0,0,0); 16-byte aligned */
    void *ids_dev;          /* n x 2 int32 (primitive id, triangle in the primitive), -1,-1 for a miss; 8-byte aligned */
    void *point_dev;        /* n x float4: the contact point on the SCENE triangle, w = 1; a miss is zeros.  16-byte aligned.  May be NULL */
    void *qpoint_dev;       /* n x float4: the witness point on the QUERY triangle in its rest pose, w = 1; a miss is zeros.  16-byte aligned.  May be NULL */
    void *hip_stream;       /* as ArtRayCast: NULL = the context's cast stream */
    uint32_t n, cull_mask, flags, reserved;   /* n = 0 is legal: nothing is enqueued; cull_mask 0..0xFF; flags, reserved: must be 0 */
} ArtTriCast;               /* 64 bytes */
int32_t art_cast_triangles(ArtContext *ctx, const ArtTriCast *c);

/* get_color_output_image / get_output_depth_image / get_output_normal_image (vk_rt_lightning_shadows.rs:161-183):
 * fp32 RGBA colour (the value passed to imageStore, before the reference's lossy image formats), fp32 depth,
 * fp32 RGBA normal; row-major full frame, of the most recently traced frame.  Host copies (synchronising) and raw device
 * pointers (with a frame ring: valid until frames_in_flight - 1 more frames have been traced). */
int32_t art_read_color(ArtContext *ctx, void *dst, size_t bytes);
int32_t art_read_depth(ArtContext *ctx, void *dst, size_t bytes);
int32_t art_read_normal(ArtContext *ctx, void *dst, size_t bytes);
int32_t art_device_color(ArtContext *ctx, void **dev_ptr, size_t *bytes);
int32_t art_device_depth(ArtContext *ctx, void **dev_ptr, size_t *bytes);
int32_t art_device_normal(ArtContext *ctx, void **dev_ptr, size_t *bytes);

/* screen-tile sharding (new functionality, BASELINE.json): compact per-shard colour tiles for the RCCL gather, and
 * the un-tile step run by the root on the gathered buffer.  tile = 32x32 px of RGB32F = 12 KiB each: the colour without its alpha, which is
 * the constant 1 of imageStore(vec4(rho, 1)) (raytrace.rgen.glsl:197) -- three quarters of the bytes on the links, nothing lost; the un-tile writes
 * the RGBA32F frame. */
int32_t art_shard_tile_count(ArtContext *ctx, uint32_t *owned, uint32_t *padded);
/* host-only (no device needed): the row-major ids of the tiles shard_rank owns for a width x height frame cut for shard_count shards with
 * ArtConfig.root_relief = root_relief, in the order they sit in its compact buffer; *owned = their number, *padded = the largest count
 * over all shards (the per-rank gather size).  tiles may be NULL to query the counts; cap = capacity of tiles. */
int32_t art_shard_layout(uint32_t width, uint32_t height, uint32_t shard_count, uint32_t shard_rank, uint32_t root_relief, uint32_t *tiles,
                         uint32_t cap, uint32_t *owned, uint32_t *padded);
int32_t art_device_color_tiles(ArtContext *ctx, void **dev_ptr, size_t *bytes);
/* frame_dev NULL = the context's colour buffer; hip_stream NULL = the latest frame's stream */
int32_t art_untile_gathered(ArtContext *ctx, const void *gathered_dev, uint32_t shard_count, void *frame_dev, void *hip_stream);
/* what a caller that sizes buffers around a context needs to know (the multi-GPU frame below does) */
typedef struct ArtLayout {
    uint32_t width, height;
    uint32_t frames_in_flight;   /* ring slots */
    uint32_t frames_per_launch;  /* frames one art_trace traces = frames per ring slot */
    uint32_t shard_rank, shard_count;
    uint32_t tiles_owned, tiles_padded; /* 32x32 tiles this shard renders; the largest count over all shards (the per-rank gather size) */
    uint32_t tile_bytes;         /* bytes of one tile in the compact tile buffer: 12288 (RGB32F) or 4096 (ART_FLAG_PACKED_TILES); 0: the context writes none */
    uint32_t reserved;
} ArtLayout;
int32_t art_get_layout(ArtContext *ctx, ArtLayout *out);
/* ---- the sharded frame as one surface (new functionality, BASELINE.json north_star: "frames shard by screen tile across the 8 GPUs of one node
 * with an RCCL gather of the HDR buffer over xGMI"; the reference renders on one queue of one device, renderer.rs:188) ----------------------------
 * One process per GPU.  Every process creates its context with the shard art_mgpu_shard gives it, loads the same scene, and creates an ArtMgpu
 * from the SAME 128-byte id (rank 0 makes it with art_mgpu_unique_id and passes it on by whatever channel the host has: a file, a socket,
 * MPI, torch.distributed).  Then every rank calls, frame after frame and in the same order,
 *     art_set_camera(ctx, ..)   (all ranks the same camera)        art_mgpu_trace(mg)
 * and the assembled frames are found behind art_mgpu_flush / art_mgpu_read_frame (on rank 0, or with ART_MGPU_ROOT_SPREAD frame f on rank f mod world).
 * Inside: the rank's share is traced into a ring of compact tile buffers (4 per ring slot, written in turn); the tiles of `launches_per_gather`
 * launches travel as ONE exchange -- an ncclGather (RCCL, rccl.h:745) to rank 0, or one ncclGroupStart .. ncclGroupEnd of ncclSend / ncclRecv that
 * takes every frame to its own root -- on a stream of their own, submitted by the host once it has SEEN the group's frames finish (art_frames_done:
 * no device-side wait in front of the collective or of the next frames -- such waits cost the frames in flight their L2 contents, profiles/README.md
 * r1n), and one launch un-tiles a root's frames of the group.  The payload is the context's tile format: RGB32F -- the
 * HDR buffer, 12 B per pixel (its alpha is the constant 1) -- by default, B10G11R11 words with ART_FLAG_PACKED_TILES.
 * RCCL is loaded at art_mgpu_create (dlopen of librccl.so.1: libart itself does not link it); ART_E_NO_DEVICE if it cannot be. */
typedef struct ArtMgpu ArtMgpu;
#define ART_MGPU_ID_BYTES 128
#define ART_MGPU_SHARED 0u     /* rank 0 traces a share AND receives / un-tiles every frame */
#define ART_MGPU_DEDICATED 1u  /* rank 0 only receives and un-tiles; ranks 1..world-1 trace 1/(world-1) each */
#define ART_MGPU_RCCL 0u
#define ART_MGPU_HOST_EXCHANGE 1u /* the collective is the caller's function (rehearsals on one GPU, where RCCL refuses two ranks per device; other fabrics) */
#define ART_MGPU_ROOT_RANK0 0u   /* every frame is assembled on rank 0: one ncclGather per group of launches */
#define ART_MGPU_ROOT_SPREAD 1u  /* frame f (counted over the job, from 0) is assembled on rank f mod world: per group one ncclGroupStart .. ncclGroupEnd of ncclSend /
                                    ncclRecv, i.e. every frame's gather at once.  xGMI is point to point, one link per pair of GPUs: a single root receives over its own
                                    links only (2 GPUs: a half frame of RGB32F tiles, 12.4 MB at 1080p, per frame over ONE link); spread roots use every link in both
                                    directions.  art_mgpu_device_frame / art_mgpu_read_frame then give, on every rank, the newest frame that fell to it. */
/* must leave, ordered before anything enqueued on hip_stream afterwards, every rank's `bytes` bytes (rank order) in recv_dev on rank `root`
 * (recv_dev is NULL elsewhere); send_dev is complete when it is called, and nothing enqueued earlier on hip_stream still reads recv_dev (the library has
 * waited for the un-tile of the previous group).  Returns 0 or an error the library passes on as ART_E_HIP -- after which the ArtMgpu only reports that
 * error (frames of the failed group are lost; destroy it). */
typedef int32_t (*ArtMgpuExchangeFn)(void *user, const void *send_dev, size_t bytes, void *recv_dev, uint32_t root, void *hip_stream);
typedef struct ArtMgpuConfig {
    uint32_t rank, world;        /* this process; processes (= GPUs) of the job */
    uint32_t compositor;         /* ART_MGPU_SHARED | ART_MGPU_DEDICATED */
    uint32_t launches_per_gather;/* ring slots per collective; 0 = all of the ring (one collective per trip); rounded down to a divisor of the ring */
    uint32_t tile_buffers;       /* compact tile buffers per ring slot, 1..8; 0 = 4 */
    uint32_t transport;          /* ART_MGPU_RCCL | ART_MGPU_HOST_EXCHANGE */
    ArtMgpuExchangeFn exchange;  /* ART_MGPU_HOST_EXCHANGE only */
    void *exchange_user;
    uint32_t roots;              /* ART_MGPU_ROOT_RANK0 | ART_MGPU_ROOT_SPREAD (ART_MGPU_SHARED only) */
    uint32_t reserved;
} ArtMgpuConfig;
/* host only: the shard (ArtConfig.shard_rank / shard_count) rank `rank` of `world` creates its context with */
int32_t art_mgpu_shard(uint32_t rank, uint32_t world, uint32_t compositor, uint32_t *shard_rank, uint32_t *shard_count);
int32_t art_mgpu_unique_id(uint8_t id[ART_MGPU_ID_BYTES]);
/* ctx: built scene, final extent, frames in flight and frames per launch (change none of them while the ArtMgpu lives).  Collective: every rank calls it. */
int32_t art_mgpu_create(ArtContext *ctx, const ArtMgpuConfig *cfg, const uint8_t id[ART_MGPU_ID_BYTES], ArtMgpu **out);
/* one launch of this rank's share (art_trace: frames_per_launch frames with the context's current camera[s]) + its part of the exchange. */
int32_t art_mgpu_trace(ArtMgpu *mg);
/* every frame traced so far has been gathered and (rank 0) un-tiled when it returns.  Collective. */
int32_t art_mgpu_flush(ArtMgpu *mg);
/* a root (rank 0; every rank with spread roots), after art_mgpu_flush: the most recently traced frame it assembled (width x height RGBA32F, or B10G11R11 words with packed tiles) */
int32_t art_mgpu_device_frame(ArtMgpu *mg, void **dev_ptr, size_t *bytes);
int32_t art_mgpu_read_frame(ArtMgpu *mg, void *dst, size_t bytes);
/* frames traced / gathers submitted so far, and how many launches travel per gather */
int32_t art_mgpu_counts(ArtMgpu *mg, uint64_t *launches_traced, uint64_t *gathers, uint32_t *launches_per_gather);
/* before art_destroy of its context (it unbinds the tile buffers it owns from the context's ring slots) */
int32_t art_mgpu_destroy(ArtMgpu *mg);

int32_t art_get_stats(ArtContext *ctx, ArtStats *out);
/* ---- GLB ingest: the step right before the path (model_reader/gltf_model_reader.rs), host only ------------------ */
typedef struct ArtGlb ArtGlb;
/* MeshAttributeType / TextureType bits (model_reader.rs:5-20) */
#define ART_ATTR_VERTICES 1u
#define ART_ATTR_TEX_COORDS 2u
#define ART_ATTR_NORMALS 4u
#define ART_ATTR_TANGENTS 8u
#define ART_ATTR_INDICES 16u
#define ART_TEX_ALBEDO 1u
#define ART_TEX_ORM 2u
#define ART_TEX_NORMAL 4u
#define ART_TEX_EMISSIVE 8u
/* PrimitiveCopyInfo (model_reader.rs:52-72); image_format: 0 R8, 1 R8G8, 2 R8G8B8, 3 R8G8B8A8, 4 B8G8R8, 5 B8G8R8A8, 6..9 the R16 family */
typedef struct ArtGlbCopyInfo {
    uint64_t mesh_buffer_offset, mesh_size;
    uint64_t indices_buffer_offset, indices_size;
    uint64_t image_buffer_offset, image_size;
    uint32_t single_mesh_element_size, single_index_size;
    uint32_t image_format, image_width, image_height, image_mip_levels, image_layers, reserved;
} ArtGlbCopyInfo;
const char *art_glb_last_error(void);
/* GltfModelReader::open (gltf_model_reader.rs:55-150): coerce_format 0 none, 1 R8G8B8A8, 2 B8G8R8A8 (what VkModel asks for), 3 B8G8R8 */
int32_t art_glb_open(const char *path, int32_t normalize_vectors, int32_t coerce_format, ArtGlb **out);
int32_t art_glb_close(ArtGlb *glb);
int32_t art_glb_primitive_count(ArtGlb *glb, uint32_t *n);
/* the material of a primitive: mode 0 OPAQUE, 1 MASK, 2 BLEND (alphaMode); cutoff = alphaCutoff (0.5 by default); base_color_has_alpha = the base-colour image as
 * decoded has an alpha channel (1) or not (0: a coerced image gets alpha 0 in every texel).  art_scene_add_glb applies none of it (art_scene_set_alpha_cutoff does). */
int32_t art_glb_primitive_alpha(ArtGlb *glb, uint32_t primitive, int32_t *mode, float *cutoff, int32_t *base_color_has_alpha);
/* copy_model_data_to_ptr (:156-281): dst NULL = sizing pass; *total = bytes the copy needs */
int32_t art_glb_copy_model_data(ArtGlb *glb, uint32_t attr_mask, uint32_t tex_mask, void *dst, size_t cap, ArtGlbCopyInfo *infos,
                                uint32_t n_infos, size_t *total);
/* get_primitives_bounding_sphere (:283-399) */
int32_t art_glb_bounding_sphere(ArtGlb *glb, float center[3], float *radius);
/* permute_pixels (:542-573): map[s] = destination byte of source byte s, or -1 */
int32_t art_glb_permute_pixels(const uint8_t *src, size_t src_len, uint32_t src_texel, const int32_t *map, uint32_t map_len,
                               uint32_t dst_texel, uint8_t *dst, size_t dst_cap);
/* add_model (renderer.rs:346 -> vk_model.rs:494-528): every primitive of the GLB into the scene */
int32_t art_scene_add_glb(ArtContext *ctx, ArtGlb *glb, const float model3x4[12], uint32_t *first_primitive_id, uint32_t *n_primitives);

#ifdef __cplusplus
}
#endif
#endif /* ART_H */
