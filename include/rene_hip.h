/*
 * rene_hip.h -- C ABI of the MI355X-native render path for hatoo/rene.
 *
 * The reference (Rust + Vulkan-RT) has no FFI seam of its own: the render path is inlined in
 * `main()` (rene/src/main.rs:209-1687).  The natural seam, and the one this library implements, is
 *
 *     flat `Scene` tables in  (rene/src/scene.rs:36-49, consumed by
 *                              SceneBuffers::new, rene/src/main.rs:2910-3336)
 *     3 accumulation layers out (RGBA32F array image, rene/src/main.rs:383-408,
 *                              read back at rene/src/main.rs:1453-1623)
 *
 * Every struct below is a plain-old-data restatement of one reference table; the comment on each
 * names the reference type it replaces.  No C++ / torch / HIP types appear in any signature, so a
 * Rust host binds this with `extern "C"` + `#[repr(C)]` (see INTEGRATION.md for the stub).
 *
 * Conventions: all matrices are column-major f32 (glam `Mat4::to_cols_array`, `Affine3A` as
 * x_axis,y_axis,z_axis,translation); all indices are u32; every function returns 0 on success and
 * a negative `rene_status` otherwise, with a thread-local message behind `rene_last_error()`.
 * Nothing in this library aborts or throws across the boundary (the reference `unwrap()`s every
 * Vulkan call, rene/src/main.rs passim).
 */
#ifndef RENE_HIP_H
#define RENE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RENE_ABI_VERSION 7u

typedef enum rene_status {
  RENE_OK = 0,
  RENE_ERR_INVALID_ARGUMENT = -1,
  RENE_ERR_INVALID_SCENE = -2,
  RENE_ERR_DEVICE = -3,          /* a HIP call failed; message carries hipGetErrorString */
  RENE_ERR_UNSUPPORTED = -4,     /* e.g. GIF / TIFF / WebP textures, tiled or DWA-compressed EXR files */
  RENE_ERR_OUT_OF_MEMORY = -5,
  RENE_ERR_IO = -6,
  RENE_ERR_PARSE = -7
} rene_status;

/* ---- enumerations; numeric values equal the reference's #[repr(u32)] discriminants ---------- */

/* ShaderOffset, rene/src/main.rs:41-45 */
enum { RENE_SHAPE_TRIANGLE = 0, RENE_SHAPE_SPHERE = 1 };
/* MaterialType, rene-shader/src/material.rs:52-63 */
enum {
  RENE_MATERIAL_NONE = 0, RENE_MATERIAL_MATTE = 1, RENE_MATERIAL_GLASS = 2,
  RENE_MATERIAL_SUBSTRATE = 3, RENE_MATERIAL_METAL = 4, RENE_MATERIAL_MIRROR = 5,
  RENE_MATERIAL_UBER = 6, RENE_MATERIAL_PLASTIC = 7
};
/* TextureType, rene-shader/src/texture.rs:22-29 */
enum { RENE_TEXTURE_SOLID = 0, RENE_TEXTURE_CHECKERBOARD = 1, RENE_TEXTURE_IMAGEMAP = 2,
       RENE_TEXTURE_SCALE = 3 };
/* AreaLightType, rene-shader/src/area_light.rs:9-13 */
enum { RENE_AREA_LIGHT_NULL = 0, RENE_AREA_LIGHT_DIFFUSE = 1 };
/* LightType, rene-shader/src/light.rs:19-21 */
enum { RENE_LIGHT_DISTANT = 0 };
/* Integrator, rene/src/scene/intermediate_scene.rs:186-190 */
enum { RENE_INTEGRATOR_PATH = 0, RENE_INTEGRATOR_VOLPATH = 1 };
/* accumulation layers, rene-shader/src/lib.rs:165-172, 210, 226, 230-231 */
enum { RENE_LAYER_RADIANCE = 0, RENE_LAYER_NORMAL = 1, RENE_LAYER_ALBEDO = 2, RENE_LAYER_COUNT = 3 };

/* ---- scene tables ---------------------------------------------------------------------------- */

/* Vertex, rene-shader/src/lib.rs:883-890 (position, normal, uv); packed to 32 B here (the
 * reference's Vec3A padding carries no information). */
typedef struct rene_vertex {
  float position[3];
  float normal[3];
  float uv[2];
} rene_vertex;

/* TriangleMesh, rene/src/scene/intermediate_scene.rs:149-153.  Indices are mesh-local; the
 * library rebases them the way SceneBuffers::new does (rene/src/main.rs:2943-2963). */
typedef struct rene_mesh {
  const rene_vertex* vertices;
  const uint32_t* indices;
  uint32_t n_vertices;
  uint32_t n_indices; /* multiple of 3 */
} rene_mesh;

/* TlasInstance, rene/src/scene.rs:25-34.  `matrix` is the Affine3A object-to-world transform
 * (for spheres already multiplied by scale(radius), rene/src/scene.rs:418-423). */
typedef struct rene_instance {
  uint32_t shape;           /* RENE_SHAPE_* */
  int32_t mesh_index;       /* blas_index; -1 for spheres */
  uint32_t material_index;
  uint32_t area_light_index;
  uint32_t interior_medium_index;
  uint32_t exterior_medium_index;
  float matrix[12];         /* x_axis, y_axis, z_axis, translation */
} rene_instance;

/* EnumMaterial, rene-shader/src/material.rs:43-70.  Field use per type follows the reference's
 * `new_data` constructors (material.rs:107-115, 138-152, 228-242, 319-326, 353-360, 495-517,
 * 642-657). */
typedef struct rene_material {
  uint32_t type;
  uint32_t u0[4];
  uint32_t u1[4];
  float v0[4];
} rene_material;

/* EnumTexture, rene-shader/src/texture.rs:14-36; field use per texture.rs:62-96. */
typedef struct rene_texture {
  uint32_t type;
  uint32_t u0[4];
  float v0[4];
} rene_texture;

/* EnumAreaLight, rene-shader/src/area_light.rs:21-33 */
typedef struct rene_area_light {
  uint32_t type;
  float v0[4]; /* L.rgb, 0 */
} rene_area_light;

/* EnumLight, rene-shader/src/light.rs:8-28.  Distant: v0 = normalize(from - to), v1 = L
 * (light.rs:43-50). */
typedef struct rene_light {
  uint32_t type;
  float v0[4];
  float v1[4];
} rene_light;

/* EnumMedium, rene-shader/src/medium.rs:47-72.  Homogeneous: v0 = sigma_a.rgb, g; v1 = sigma_s.rgb, 0
 * (medium.rs:78-84).  Only the volumetric integrator reads media. */
enum { RENE_MEDIUM_VACUUM = 0, RENE_MEDIUM_HOMOGENEOUS = 1 };
typedef struct rene_medium {
  uint32_t type;
  float v0[4];
  float v1[4];
} rene_medium;

/* Image, rene/src/scene/image.rs:1-19: linear RGBA32F, row 0 first. */
typedef struct rene_image {
  const float* rgba;
  uint32_t width;
  uint32_t height;
} rene_image;

/* Uniform, rene-shader/src/lib.rs:90-102.  `projection_inv` is PerspectiveCamera.projection, i.e.
 * Mat4::perspective_lh(fov, aspect, 0.01, 1000).inverse() (rene/src/scene.rs:163-164);
 * lights_len / emit_object_len / emit_primitives are derived by the library
 * (rene/src/scene.rs:166, rene/src/main.rs:3278-3280). */
typedef struct rene_uniform {
  float camera_to_world[16];
  float background_matrix[16];
  float background_color[4];
  float projection_inv[16];
  uint32_t background_texture;
} rene_uniform;

/* Scene, rene/src/scene.rs:36-49 (+ Film, intermediate_scene.rs:155-160).  All pointers are
 * borrowed for the duration of the call they are passed to. */
typedef struct rene_scene_desc {
  uint32_t struct_size;   /* sizeof(rene_scene_desc), ABI guard */
  uint32_t integrator;    /* RENE_INTEGRATOR_* */
  uint32_t xresolution;
  uint32_t yresolution;
  rene_uniform uniform;
  uint32_t n_instances;
  uint32_t n_meshes;
  uint32_t n_materials;
  uint32_t n_textures;
  uint32_t n_area_lights;
  uint32_t n_lights;
  uint32_t n_images;
  const rene_instance* instances;
  const rene_mesh* meshes;
  const rene_material* materials;   /* [0] is the None sentinel, rene/src/scene.rs:109 */
  const rene_texture* textures;     /* [0] is solid white, rene/src/scene.rs:113-116 */
  const rene_area_light* area_lights; /* [0] is the Null sentinel, rene/src/scene.rs:110 */
  const rene_light* lights;
  const rene_image* images;
  const rene_medium* mediums;       /* [0] is the Vacuum sentinel, rene/src/scene.rs:111; may be NULL when n_mediums == 0 */
  uint32_t n_mediums;
  uint32_t reserved;
} rene_scene_desc;

/* ---- render options (additive; the reference hard-codes these, rene/src/main.rs:77-81, 1301) - */

#define RENE_DEFAULT_SEED 0x52454E45u /* "RENE" */
#define RENE_TILE_SIZE 32u

enum {
  RENE_FLAG_COUNTERS = 1u << 0, /* also count BVH node visits / primitive tests (slower kernel) */
  RENE_FLAG_NO_AOV = 1u << 1,   /* skip layers 1-2 (first-hit normal/albedo) */
  RENE_FLAG_FORCE_BVH = 1u << 2, /* traverse the BVH even when the scene qualifies for the small-scene item loop */
  RENE_FLAG_SINGLE_LEVEL = 1u << 3, /* one work item per pixel per launch (no long/short split; same results, for A/B tests) */
  RENE_FLAG_NO_RESTART = 1u << 4, /* BVH scenes: use the plain while-while kernel instead of the traversal-restart one (A/B tests) */
  RENE_FLAG_DYNAMIC_FIRST = 1u << 5, /* accepted and ignored: every work batch comes from the atomic counter (a statically owned
                                        first batch made a launch depend on all of its waves being resident) */
  RENE_FLAG_WAVEFRONT = 1u << 6, /* BVH scenes: the stage-separated wavefront integrator (wavefront.inc) instead of the traversal-restart megakernel */
  RENE_FLAG_FP16_PAYLOAD = 1u << 8, /* with RENE_FLAG_WAVEFRONT: a path slot keeps its ray direction and throughput as fp16 (BASELINE config 5's
                                       "fp16 ray payload"): 100 instead of 116 bytes per slot and round trip; origin, distances, sums and
                                       random streams stay fp32 / u32.  The image then differs from the fp32 payload's within the
                                       tolerance tests/test_gpu_scenes.py states; ignored by the default integrators, whose ray
                                       payload never leaves the registers */
  RENE_FLAG_OVERLAP = 1u << 7 /* accepted and ignored since ABI v4.  (Until v3 consecutive rene_render launches alternated between
                                 two streams so that one started while the previous drained its longest paths.  One launch now
                                 renders any number of frames in short work items, so a job is ONE rene_render call with no tail
                                 between launches to hide, and no launch ever waits for another: the occasional stall of the
                                 two-stream scheme -- docs/history.md section 4g -- has nothing left to come from.) */
  ,
  RENE_FLAG_FRAME_GROUPS = 1u << 9 /* accepted and ignored since ABI v5: what it asked for is how every context renders.  A pixel's frames are
                                      EIGHT independent chains -- global frame f belongs to chain f % 8 (under RENE_SHARD_FRAMES: (f / shard_count) % 8),
                                      each chain summed in frame order into an image of its own, across rene_render calls -- and the image a call hands
                                      out (rene_download, rene_framebuffer, rene_reduce, rene_gather_tiles, the caller's opts.framebuffer after rene_sync)
                                      is ((c0 + c1) + c2) + ... + c7.  The reference adds every frame onto the last (rene/src/main.rs:1315-1397), which
                                      on a persistent kernel makes a pixel's frames one sequential chain: a job could not end before its most expensive
                                      pixel had been through all its frames (rene's teapot scene at 8192 spp ended 13 % after its median wave) and a
                                      tile shard had fewer chains than the chip has lanes.  The rule is on the frame NUMBER, so the image is bit-identical
                                      however a job is cut into calls, launches, work items and tile shards, as before; it differs from the strict
                                      frame order only in the rounding of the regrouped fp32 sums (max 4e-5 of the image's maximum at 1024 - 8192 spp). */
};
enum { RENE_SHARD_TILES = 0, RENE_SHARD_FRAMES = 1 };

typedef struct rene_opts {
  uint32_t struct_size;  /* sizeof(rene_opts) */
  uint32_t seed;         /* master seed; frame k uses the k-th next_u32() of PCG32si::new(seed) */
  int32_t device;        /* HIP device ordinal */
  uint32_t flags;        /* RENE_FLAG_* */
  uint32_t shard_mode;   /* RENE_SHARD_* */
  uint32_t shard_rank;   /* this context renders tiles (or frames) with index % shard_count == shard_rank */
  uint32_t shard_count;  /* 0 or 1 = unsharded */
  uint32_t reserved;
  void* framebuffer;     /* optional caller-owned DEVICE buffer of 3*yres*xres*4 floats, else NULL: where the image is handed out.  The
                            library writes it whenever launches are waited for (rene_sync, rene_download, rene_get_stats,
                            rene_framebuffer, rene_reduce, rene_gather_tiles): r, g, b = the sums of the frames rendered so far
                            (the eight frame chains added, see RENE_FLAG_FRAME_GROUPS), the fourth float 0; zero it through rene_reset */
  void* stream;          /* optional hipStream_t to launch on, else NULL (library-owned stream) */
} rene_opts;

/* Device counters; a "ray" is one traversal query (SURVEY section 8 d). */
typedef struct rene_stats {
  uint64_t rays_closest;  /* rene-shader/src/lib.rs:195-207 */
  uint64_t rays_shadow;   /* lib.rs:245-258 */
  uint64_t rays_emitter;  /* lib.rs:301-314 */
  uint64_t paths;         /* raygen invocations */
  uint64_t bounces;       /* loop iterations that shaded a hit (path-state round trips) */
  uint64_t hits;          /* closest hits shaded */
  uint64_t adds;          /* add_image calls, lib.rs:165-172 */
  uint64_t node_visits;   /* only with RENE_FLAG_COUNTERS */
  uint64_t prim_tests;    /* only with RENE_FLAG_COUNTERS */
  uint64_t frames;        /* frames rendered so far (per context) */
  uint64_t launches;      /* kernel launches so far (a launch that had to be replayed after dropped work items counts again) */
  double kernel_ms;       /* sum of HIP-event durations of those launches */
  double last_launch_ms;
  double sclk_mhz;        /* engine clock while those launches ran, measured by the kernels (shader-clock ticks per tick of the
                             constant 100 MHz clock over the lifetime of one wave per launch); 0 before the first launch (ABI v4) */
} rene_stats;

/* One closest-hit record (what Vulkan traversal hands the hit shaders: t, instance, primitive,
 * barycentrics; rene-shader/src/lib.rs:892-905). */
typedef struct rene_hit {
  float t;               /* < 0: miss */
  float u, v;
  uint32_t instance;
  uint32_t primitive;
} rene_hit;

/* What rene_create would build for a scene; filled by rene_scene_pack_info without touching the
 * GPU (host-side validation + flattening + BVH build only). */
typedef struct rene_pack_info {
  uint32_t n_instances;
  uint32_t n_triangles;      /* world-space triangles after instancing is flattened */
  uint32_t n_spheres;
  uint32_t n_nodes_main, n_slots_main, depth_main;
  uint32_t n_nodes_emit, n_slots_emit, depth_emit;
  uint32_t features;         /* kernel specialisation bits: 1 spheres, 2 general BSDFs, 4 textures, 8 distant lights, 16 background,
                                32 multi-lobe materials, 64 wave-coherent item loop (no BVH), 128 volpath; for single-lobe general
                                scenes also what is absent: 256 no Glass / Mirror, 512 no Substrate, 1024 no Metal; 2048 no emit objects */
  uint32_t emit_object_len;  /* rene/src/main.rs:3279 */
  uint32_t lights_len;       /* rene/src/scene.rs:166 */
  uint64_t device_bytes;     /* HBM the scene tables will occupy (framebuffer excluded) */
  uint32_t n_items_main;     /* items the small-scene loop visits per ray (0: the scene uses the BVH), main / emitter-only */
  uint32_t n_items_emit;
} rene_pack_info;

/* The device memory a context of this scene and these options allocates; filled by rene_plan_memory without touching the GPU.
 * Chains and versions cover the pixel slots of the tiles the context owns (all tiles unsharded, every shard_count-th under
 * RENE_SHARD_TILES): n_slots = owned tiles * 1024. */
typedef struct rene_memory_plan {
  uint64_t chain_bytes;    /* the frame chains' running sums: 8 chains * 3 layers * 16 bytes * n_slots */
  uint64_t version_bytes;  /* the work items' version words: 8 chains * 4 bytes * n_slots */
  uint64_t image_bytes;    /* the image handed out, 3 layers * W * H * 16 bytes; 0 with a caller-owned framebuffer */
  uint64_t scene_bytes;    /* the scene's tables */
  uint64_t queue_bytes;    /* the wavefront integrator's path queues (RENE_FLAG_WAVEFRONT), else 0 */
  uint64_t total_bytes;    /* all of the above and the context's counters */
} rene_memory_plan;

typedef struct rene_ctx rene_ctx;

/* ---- render path ----------------------------------------------------------------------------- */

/* Replaces SceneBuffers::new + pipeline/SBT/descriptor setup (rene/src/main.rs:513-1199): flatten,
 * build the BVHs, upload, clear the accumulation image (main.rs:1229-1237). */
int rene_create(const rene_scene_desc* scene, const rene_opts* opts, rene_ctx** out);

/* Replaces the trace loop (rene/src/main.rs:1315-1397): render frames
 * [first_frame, first_frame + n_frames) and add them into the accumulation layers.  Asynchronous
 * on the context's stream; ordered with later calls on the same context.  ONE persistent launch per call (requests beyond
 * 65 536 frames are cut): a whole job is best rendered by one call -- every call ends on the longest paths of its last work
 * items -- and the image does not depend on how a job is cut into calls (bit-identical). */
int rene_render(rene_ctx* ctx, uint32_t first_frame, uint32_t n_frames);

/* Waits for everything queued on the context (queue_wait_idle, main.rs:1389). */
int rene_sync(rene_ctx* ctx);

/* Replaces layer readback + f32_4_to_3 (main.rs:1453-1619): copies layer `layer` as tightly packed
 * RGB (channels == 3) or RGBA (channels == 4) f32 rows, top row first, un-averaged sums (under adaptive sampling, rene_set_active_tiles
 * below, every tile's sums over its own N_t frames: rene_tile_frames, rene_download_mean). */
int rene_download(rene_ctx* ctx, int layer, int channels, float* dst, size_t dst_floats);

/* Zero the accumulation layers and the counters (main.rs:1229-1237). */
int rene_reset(rene_ctx* ctx);

/* Optional, before rendering: picks how long the work items of a launch of `n_frames` frames are (no reference counterpart;
 * rene dispatches one frame at a time, main.rs:1355-1372).  Few, long items cost the least bookkeeping; short ones balance
 * scenes whose pixels differ widely in cost and end the launch on a short tail.  Renders three launches of `n_frames` frames
 * per candidate (one item per pixel and launch, then items of 256, 128, ... 16 frames), keeps the fastest, then resets the
 * context like rene_reset.  Untuned contexts cut a pixel's frames into sixteen items per launch (of at least 64 frames) with the
 * small-scene kernels and 32 (of at least 16, the last ones halving) with the BVH kernels, over its eight frame chains.  The choice
 * changes no bit of any image -- a chain's frames are added in the same order however they are cut. */
int rene_tune(rene_ctx* ctx, uint32_t n_frames);

/* Device address of the accumulation image [3][yres][xres][4] f32 (for callers that run their own exchange, e.g.
 * torch.distributed; rene_reduce / rene_gather_tiles below do it inside the library).  Waits for the launches issued so far: the
 * image is the frame chains added together, which happens then.  Un-averaged sums, like rene_download's: under adaptive sampling every tile's
 * over its own N_t frames (rene_tile_frames). */
int rene_framebuffer(rene_ctx* ctx, void** device_ptr, size_t* n_floats);

/* ---- denoiser `atrous` (ABI v7; build-defined: the reference hands its image to OIDN / OptiX, rene/src/main.rs:1625-1647, whose networks
 * this build does not carry) ------------------------------------------------------------------------------------------------------
 * An edge-avoiding a-trous wavelet filter (Dammertz et al. 2010; the spatial half of SVGF, Schied et al. 2017) on the device, guided by the
 * first-hit normal and albedo layers and by the variance of the pixel's mean -- which the eight frame chains (RENE_FLAG_FRAME_GROUPS) give for
 * nothing: eight independent sub-means per pixel.  With the chains' radiance sums C_c, their frame counts n_c (N their sum, k the chains with
 * n_c > 0), S0 = ((C_0 + C_1) + ...) + C_7 and S1, S2 the normal and albedo layers' sums, lum(v) = 0.2126 r + 0.7152 g + 0.0722 b and
 * h = (1/16, 1/4, 3/8, 1/4, 1/16):
 *   1. guides alb = S2 / N, nrm = S1 / N (not renormalised: its length carries edge coverage), den = alb + albedo_floor per channel;
 *   2. demodulated colour d = (S0 / N) / den, l = lum(d);
 *   3. variance of the mean: l_c = lum((C_c / n_c) / den) for chains with n_c > 0, var = sum_c (n_c / N) (l_c - l)^2 / (k - 1);
 *   4. iteration i = 0 .. iterations - 1, step s = 2^i, from (col, var) = (d, var):
 *        g = 3x3 filter of var with weights (1 2 1) x (1 2 1) / 16, taps outside the image skipped and the weights renormalised,
 *        sd = sigma_luminance * sqrt(max(g, 0));
 *        for the 25 taps q = p + s (dx, dy), dx, dy in -2 .. 2, taps outside the image skipped:
 *          e = |nrm_p - nrm_q|^2 / sigma_normal2 + |alb_p - alb_q|^2 / sigma_albedo2
 *              + |lum(col_p) - lum(col_q)| / (sd_p + relative_floor (|lum(col_p)| + |lum(col_q)|) + 1e-12),
 *          w = h[dx + 2] h[dy + 2] exp(-e);
 *        col'_p = sum w col_q / sum w,  var'_p = sum w^2 var_q / (sum w)^2;
 *   5. radiance out = col * den * N -- un-averaged sums like those of rene_download, so that rene_to_rgb8(out, n_floats, N, rgb) applies
 *      unchanged; the variance plane handed out is the UNFILTERED var of step 3 (a diagnostic).
 * All of it in fp32.  The accumulation state is read, never written: rene_download, the chains and later frames are bit for bit what they are
 * without the call.  The filter is NOT energy preserving: a bright, noisy pixel is pulled towards dark neighbours that in turn reject it, so
 * image means drop, most around small emitters (DESIGN.md section 4c has figures; rene_resolve_robust below is the call that removes fireflies
 * as such, from the unfiltered image).  With RENE_FLAG_NO_AOV the guides are zero and the filter
 * is guided by luminance alone. */
typedef struct rene_denoise_params {
  uint32_t struct_size;    /* sizeof(rene_denoise_params) */
  uint32_t iterations;     /* 1..8, default 5 */
  float sigma_luminance;   /* default 4 */
  float sigma_normal2;     /* default 1/64 */
  float sigma_albedo2;     /* default 1/16 */
  float albedo_floor;      /* default 0.05 (a floor of 1e-3 amplifies the noise of dark albedo: the fog scene came out worse than it went in) */
  float relative_floor;    /* default 1e-3: keeps the luminance weight defined where the variance is zero (background, covered emitters) */
  uint32_t reserved;
} rene_denoise_params;
/* the defaults above; host only */
void rene_denoise_params_default(rene_denoise_params* out);
/* Filters the frames accumulated so far (params == NULL: the defaults).  Waits for the launches issued so far, as rene_framebuffer does, runs
 * on the context's stream and returns when the result is there.  The first call allocates the filter's buffers, which rene_destroy frees and
 * rene_plan_memory does not count: RENE_DENOISE_BYTES_PER_PIXEL bytes per pixel of the image (two 16-byte records, 32 bytes of guides, the
 * 16-byte output, the 4-byte variance plane).  Every integrator and kernel family is supported -- the filter only reads chains.
 * RENE_ERR_INVALID_ARGUMENT: bad struct_size, iterations outside 1..8, a sigma or floor that is not finite and positive, frames in fewer than
 * two chains (k < 2: fewer than two frames rendered, or all of them in one chain).  RENE_ERR_UNSUPPORTED: a context with shard_count > 1 (tile
 * shards are denoised by rene_denoise_shard_prepare / rene_denoise_place_shard / rene_denoise_placed, further down), and
 * a context whose chains an exchange has consumed (rene_reduce, rene_gather_tiles) until its rene_reset, and a context whose owned tiles differ
 * in their frame counts (rene_set_active_tiles) until its rene_reset. */
#define RENE_DENOISE_BYTES_PER_PIXEL 84u
int rene_denoise(rene_ctx* ctx, const rene_denoise_params* params);
enum { RENE_DENOISED_RADIANCE = 0, RENE_DENOISED_VARIANCE = 1, RENE_DENOISED_MEAN = 2, RENE_DENOISED_TRIM = 3 };
/* The result of the last rene_denoise, rene_denoise_tiles, rene_denoise_robust or rene_denoise_tiles_robust (below), whichever ran last, rows top
 * first: the radiance as RGB or RGBA sums (channels 3 or 4, alpha 0), the variance plane (channels 1), RENE_DENOISED_MEAN (channels 3 or 4,
 * alpha 0): col * den of step 5 without the frame count, the filtered MEAN image -- after any of the calls; it is computed by this call from the
 * filter's own buffers, so rendering on after the denoise does not change it -- or RENE_DENOISED_TRIM (channels 1): (float)j per pixel, the chains
 * a robust call left out at either end, all zeros after a call that trims nothing (rene_denoise, rene_denoise_tiles) and on invalid tiles.
 * RENE_ERR_INVALID_ARGUMENT before any such call since the context was created or reset. */
int rene_download_denoised(rene_ctx* ctx, int what, int channels, float* dst, size_t dst_floats);
/* Device address of the denoised radiance [yres][xres][4] f32, like rene_framebuffer; same precondition as rene_download_denoised. */
int rene_denoised_buffer(rene_ctx* ctx, void** device_ptr, size_t* n_floats);

/* ---- denoiser `atrous`, tile by tile (build-defined; ABI v7, added symbols) --------------------------------------------------------------------
 * The filter above for the image of an adaptive job (rene_set_active_tiles, further down), whose 32 x 32 tiles stopped at different frame counts:
 * the same params, the same validation, the same buffers, and for download and device address the two calls above.  Owned tile t has the chain
 * counts n_c(t), their sum N_t and k_t, the chains with n_c(t) > 0 -- the numbers rene_estimate_noise and rene_resolve_robust derive from the first
 * frame rendered and N_t (on a context whose owned tiles all hold the same frames: the context's own counts, as rene_denoise takes them).
 *   Valid and invalid tiles.  A tile is VALID if k_t >= 2.  A pixel of an invalid tile -- a tile that never rendered, a tile with all its frames in
 *   one chain -- is treated exactly as a pixel outside the image: it is skipped as a tap, in the 25-tap sums of step 4 and in the 3 x 3 filter of the
 *   variance, the weights renormalised as at the image border; and it is not filtered itself.
 *   1 - 3. on a pixel of a valid tile: steps 1 - 3 above with N, k, n_c replaced by N_t, k_t, n_c(t).  The unfiltered variance plane
 *      (RENE_DENOISED_VARIANCE) is therefore, tile by tile, bit for bit that of rene_denoise after rene_render(first, N_t) on a context without
 *      inactive tiles; on invalid pixels it is 0.
 *   4. unchanged: the same expressions in the same order, over the taps that are inside the image AND valid.
 *   5. RENE_DENOISED_RADIANCE = (col * den) * N_t -- the unit of rene_download on that context, sums over the TILE's frames;
 *      RENE_DENOISED_MEAN = col * den, so the radiance is the mean times (float)N_t, rounded once.  Invalid pixels hand out the unfiltered image:
 *      the radiance bit for bit rene_download's, the mean bit for bit rene_download_mean's (0 where N_t == 0).
 * Even contexts: where the owned tiles all hold the same frames and k >= 2, the result equals rene_denoise's bit for bit, radiance and variance,
 * whichever pass is staged in LDS and in whichever order the workgroups take their tiles.
 * Like rene_denoise the call only reads chains, image and version words, is deterministic from run to run, independent of how the job was cut
 * into calls, and works on a context filled by rene_load_chains with per-tile counts.  It needs no memory beyond rene_denoise's
 * RENE_DENOISE_BYTES_PER_PIXEL but the table of constants the chain passes share: 76 bytes per distinct N_t and 4 bytes per tile.
 * RENE_ERR_INVALID_ARGUMENT: bad params as for rene_denoise; no valid owned tile at all.  RENE_ERR_UNSUPPORTED: shard_count > 1 (the next section); a context
 * whose chains an exchange has consumed.  A refusal leaves the context usable and the previous result downloadable. */
int rene_denoise_tiles(rene_ctx* ctx, const rene_denoise_params* params);

/* ---- denoiser `atrous` on tile shards: prepare on the shards, filter on one (build-defined; ABI v7, added symbols) -------------------------------------
 * rene_denoise and rene_denoise_tiles refuse a context with shard_count > 1: the filter needs neighbours across shards.  But only steps 1 - 3 (prepare)
 * read the frame chains, and they are strictly per pixel; steps 4 - 5 read nothing but the records prepare wrote -- 52 bytes per pixel: the 16-byte
 * record {d, var}, the two 16-byte guide records, which carry the pixel's validity and (float)N_t, and the 4-byte variance plane.  So:
 *   1. every tile shard runs rene_denoise_tiles' prepare on the tiles it owns, into a tile-packed buffer (rene_denoise_shard_prepare);
 *   2. the packed buffers travel to one context of the same film, the ROOT -- by rene_gather_denoise over the communicator, or by the caller
 *      (rene_denoise_shard_buffer / rene_download_denoise_shard, then rene_denoise_place_shard on the root, from a device or a host pointer);
 *   3. the root runs steps 4 - 5 of rene_denoise_tiles on the assembled records (rene_denoise_placed) and hands the result out through
 *      rene_download_denoised and rene_denoised_buffer, as after rene_denoise_tiles.
 * Nothing in the filter's arithmetic changes and no halo is exchanged: the result is bit for bit that of rene_denoise_tiles on an unsharded
 * context that holds the same frames (and so, on even tiles with k >= 2, that of rene_denoise), radiance, variance plane and mean, the invalid
 * tiles' unfiltered image included.  The root may be one of the shards or any other context of the same resolution: it needs no frames of its own,
 * only the filter's RENE_DENOISE_BYTES_PER_PIXEL buffers.  An unsharded context counts as a shard of one.
 *
 * The packed buffer of shard r of n (rene_denoise_shard_bytes; little endian, every part 16-byte aligned):
 *   rene_denoise_shard_header                   64 bytes: the film, the shard, the params used
 *   rene_denoise_shard_tile [n_owned]           N_t and validity of owned tile k = image tile r + k n; padded with zero bytes to a multiple of 16
 *   per owned tile k, in owned order, 53248 bytes:
 *     float rec    [1024][4]                    slot order (8 x 8 sub-blocks, the order of the frame chains): {d.rgb, var}
 *     float guides [1024][2][4]                 {nrm.xyz, alb.r}, {alb.g, alb.b, valid, (float)N_t}; an invalid tile: {S0.rgb, 0}, {0, 0, 0, 0}
 *     float var    [1024]                       the unfiltered variance of the mean
 *   A slot outside the image (ragged right and bottom tiles) holds zero bytes: the buffer is deterministic byte for byte, and tile t's block is the
 *   same bytes whichever shard layout its owner belongs to.
 *
 * The order of calls: rene_denoise_shard_prepare reads the chains, so it comes BEFORE rene_reduce / rene_gather_tiles mark the context exchanged
 * (after them it returns RENE_ERR_UNSUPPORTED until rene_reset).  A packed buffer made before stays usable afterwards: rene_denoise_shard_buffer,
 * rene_download_denoise_shard, rene_gather_denoise and rene_denoise_place_shard do not read the chains.  rene_reset discards it,
 * and with it what a rene_gather_denoise on this context left to be placed (records already placed on a root stay).
 * The trimmed variants (rene_denoise_robust, rene_denoise_tiles_robust) stay refused on shards. */
#define RENE_DENOISE_SHARD_MAGIC 0x48534e44u /* "DNSH" */
#define RENE_DENOISE_SHARD_TILE_BYTES 53248u /* 52 bytes per slot of a 32 x 32 tile */
typedef struct rene_denoise_shard_header {
  uint32_t magic;          /* RENE_DENOISE_SHARD_MAGIC */
  uint32_t header_bytes;   /* sizeof(rene_denoise_shard_header) */
  uint32_t width, height;  /* the film */
  uint32_t shard_rank, shard_count;
  uint32_t n_owned;        /* tiles in this buffer: those with index % shard_count == shard_rank */
  uint32_t reserved;
  rene_denoise_params params; /* what prepare was called with (defaults filled in): the root filters with them */
} rene_denoise_shard_header;
typedef struct rene_denoise_shard_tile {
  uint32_t n_frames;       /* N_t */
  uint32_t valid;          /* 1: k_t >= 2, the tile takes part in the filter; 0: it is handed out unfiltered */
} rene_denoise_shard_tile;
/* Bytes of the packed buffer of shard `shard_rank` of `shard_count` for a width x height film (host only, no GPU needed); 0 for an empty film,
 * a resolution above 16384, shard_count == 0 or shard_rank >= shard_count.  A shard that owns no tile has header bytes only. */
size_t rene_denoise_shard_bytes(uint32_t width, uint32_t height, uint32_t shard_rank, uint32_t shard_count);
/* Steps 1 - 3 of rene_denoise_tiles on the tiles the context owns, into the context's packed buffer (allocated by the first call, freed by
 * rene_destroy, not counted by rene_plan_memory: 52 bytes per owned pixel slot, 1 / shard_count of the unsharded filter's records).  Valid on a
 * tile shard and on an unsharded context.  The per-tile constants are derived exactly as rene_denoise_tiles derives them; params == NULL: the
 * defaults.  Like rene_denoise_tiles it waits for the launches issued so far, only reads chains and image, and is deterministic.
 * RENE_ERR_INVALID_ARGUMENT: bad params as for rene_denoise; a shard that owns tiles none of which is valid (a job of one frame).
 * RENE_ERR_UNSUPPORTED: a frame shard (RENE_SHARD_FRAMES with shard_count > 1); a context whose chains an exchange has consumed.
 * A refusal leaves the context usable and a previous packed buffer as it was. */
int rene_denoise_shard_prepare(rene_ctx* ctx, const rene_denoise_params* params);
/* The packed buffer of the last rene_denoise_shard_prepare: its device address (valid until the next prepare, rene_reset or rene_destroy) and size,
 * or a copy in host memory (dst_bytes >= that size).  RENE_ERR_INVALID_ARGUMENT before any prepare since the context was created or reset. */
int rene_denoise_shard_buffer(rene_ctx* ctx, void** device_ptr, size_t* n_bytes);
int rene_download_denoise_shard(rene_ctx* ctx, void* dst, size_t dst_bytes);
/* Places one shard's packed buffer on the root: `src` is a host pointer or a device pointer (of any device the root's can copy from), `bytes` its
 * size.  The first call allocates the filter's buffers (RENE_DENOISE_BYTES_PER_PIXEL per pixel, as rene_denoise) and a staging buffer of the
 * largest body placed so far.  A ROUND is what is placed between two completed rene_denoise_placed; placing a rank again within a round replaces
 * it.  The first placement of a round invalidates the previous result (rene_download_denoised refuses until rene_denoise_placed).
 * rene_denoise and its kin on the root use the same buffers: they discard a round in progress.
 * RENE_ERR_INVALID_ARGUMENT, with a message, and nothing placed: bytes smaller than a header or different from rene_denoise_shard_bytes of the
 * header's film and shard; a bad magic, header size, rank or tile count; a shard_count above 262144 (the tiles of the largest film); a film that is not the root's; a shard_count or params that differ from
 * those of the buffers already placed in this round; params rene_denoise would refuse. */
int rene_denoise_place_shard(rene_ctx* root_ctx, const void* src, size_t bytes);
/* Steps 4 - 5 on the records placed: the masked passes and finalize of rene_denoise_tiles with the params of the round's headers, then the result
 * is there as after rene_denoise_tiles (RENE_DENOISED_MEAN divides the invalid tiles' sums by the N_t their headers carried) and the round is over.
 * Buffers received by rene_gather_denoise are placed first.  RENE_ERR_INVALID_ARGUMENT unless every rank 0 .. shard_count - 1 has been placed in
 * this round; the message names the missing ranks, and what has been placed stays placed. */
int rene_denoise_placed(rene_ctx* root_ctx);
/* The RCCL leg, shaped like rene_gather_tiles (below): every rank of the communicator calls it after its rene_denoise_shard_prepare; a non-root rank
 * sends its packed buffer, the root receives the others' into staging.  The received buffers and the root's own are placed at the start of the
 * root's rene_denoise_placed -- inside a caller's rene_comm_group_begin / _end the receives are only enqueued when the group ends.  The context must
 * be tile-sharded with shard_count == n_ranks and shard_rank == rank; a communicator of one (an unsharded context) sends nothing and still places
 * and filters through the same kernels.  RENE_ERR_INVALID_ARGUMENT: no communicator, root out of range, no packed buffer. */
int rene_gather_denoise(rene_ctx* ctx, int root);

/* ---- noise estimate (build-defined; the reference renders a fixed 5000 samples, rene/src/main.rs:80) -------------------------------------------
 * How noisy is the image accumulated so far -- as a whole and per 32 x 32 tile -- from the same eight frame chains the denoiser takes its
 * variance from, without filtering anything.  With C_c, n_c, N, k and lum as in the denoiser's contract above:
 *   1. per owned pixel inside the image: S0 = ((C_0 + C_1) + ...) + C_7, l = lum(S0 / N), l_c = lum(C_c / n_c) for chains with n_c > 0,
 *      var = sum_c (n_c / N) (l_c - l)^2 / (k - 1) -- the denoiser's step 3 with den = 1: no albedo demodulation, no guide layers;
 *   2. per owned tile t: A_t = sum var, B_t = sum l over its n_t pixels inside the image (fp32, in a fixed order: a tile's record is the same
 *      bit for bit from run to run, however the job was cut into calls, and in an unsharded context and the tile shard that owns the tile),
 *      q_t = (A_t / n_t) / (B_t / n_t + luminance_floor)^2, tile noise = sqrt(q_t): the relative standard error of the tile's mean pixel;
 *   3. image: noise = sqrt(sum_t n_t q_t / sum_t n_t), worst_tile_noise = max_t sqrt(q_t) at tile worst_tile (the lowest such index),
 *      rel_rmse = sqrt(sum A / n) / (sum B / n + luminance_floor), n = sum_t n_t -- these sums in fp64 on the host, in tile order.
 * Numerator and denominator are averaged over the tile BEFORE they are divided.  A per-pixel ratio sd_p / (l_p + floor) is not offered: a
 * pixel's mean and its variance come from the same few frames, one bright frame raises both, and the ratio saturates near sqrt(1/8) instead of
 * halving for four times the frames (DESIGN.md section 4c has the figures).  The tile and image figures do halve, and the estimated variance
 * agrees with the empirical variance of the pixel means over master seeds within a few per cent.  Known limit: where the noise is fireflies
 * (a small bright emitter found by chance), ONE render's figure scatters widely -- on rene's veach-mis scene the ratio of the figures at 16
 * and 64 samples ranges from 1.3 to 3.3 over seeds -- so a job rendered to a target may stop early or late there
 * (rene_resolve_robust below removes such samples from the IMAGE; this figure still describes the plain mean).
 * The accumulation state is read, never written. */
typedef struct rene_noise_params {
  uint32_t struct_size;    /* sizeof(rene_noise_params) */
  uint32_t reserved0;
  float luminance_floor;   /* default 0.01; finite and positive: keeps q_t defined on black tiles */
  uint32_t reserved1;
} rene_noise_params;
/* one tile's record: A_t, B_t, n_t */
typedef struct rene_noise_tile {
  float sum_var;
  float sum_lum;
  uint32_t n_pixels;
  uint32_t reserved;
} rene_noise_tile;
typedef struct rene_noise_estimate {
  uint32_t struct_size;    /* sizeof(rene_noise_estimate) */
  uint32_t n_tiles;        /* additive: owned tiles */
  uint64_t n_pixels;       /* additive: n = sum n_t */
  double sum_var;          /* additive: sum A_t */
  double sum_lum;          /* additive: sum B_t */
  double sum_weighted_q;   /* additive: sum n_t q_t */
  uint64_t n_frames;       /* N */
  uint32_t n_chains;       /* k */
  float luminance_floor;
  double noise;            /* derived from the additive fields and the worst tile */
  double rel_rmse;
  double worst_tile_noise;
  uint32_t worst_tile;     /* ty * tiles_x + tx on the image's full tile grid, tiles_x = ceil(xresolution / 32) */
  uint32_t reserved;
} rene_noise_estimate;
/* the defaults above; host only */
void rene_noise_params_default(rene_noise_params* out);
/* Estimates the noise of the frames accumulated so far (params == NULL: the defaults).  Waits for the launches issued so far, as rene_framebuffer
 * does, runs on the context's stream and returns when *out is filled.  The first call allocates 16 bytes per owned tile, which rene_destroy
 * frees and rene_plan_memory does not count.  A RENE_SHARD_TILES shard reports the tiles it owns; the shards' estimates add.
 * RENE_ERR_INVALID_ARGUMENT: bad struct_size, a floor that is not finite and positive, frames in fewer than two chains (k < 2).
 * RENE_ERR_UNSUPPORTED: a frame shard (RENE_SHARD_FRAMES with shard_count > 1: it holds a share of every pixel's frames), and a context whose
 * chains an exchange has consumed (rene_reduce, rene_gather_tiles) until its rene_reset. */
int rene_estimate_noise(rene_ctx* ctx, const rene_noise_params* params, rene_noise_estimate* out);
/* The tile records of the last estimate on the full tiles_y x tiles_x grid, row-major (n >= tiles_y * tiles_x records at dst); tiles the
 * context does not own are zero.  RENE_ERR_INVALID_ARGUMENT before any estimate since the context was created or reset. */
int rene_download_noise_tiles(rene_ctx* ctx, rene_noise_tile* dst, size_t n);
/* Host only: the estimate of a tile-sharded job from its shards' -- the additive fields summed, the worst tile taken, the derived figures
 * recomputed.  RENE_ERR_INVALID_ARGUMENT: n == 0, a bad struct_size, parts whose n_frames or luminance_floor differ. */
int rene_noise_combine(const rene_noise_estimate* parts, size_t n, rene_noise_estimate* out);
/* Host only: the frames a job needs for `target`, by the 1 / sqrt(N) law: ceil(N (noise / target)^2), at least N, saturating at 2^32 - 1
 * (also for a target that is not positive). */
uint32_t rene_noise_frames_needed(const rene_noise_estimate* est, double target);

/* ---- adaptive sampling (build-defined; ABI v7, added symbols) ---------------------------------------------------------------------------------
 * The per-tile figures above say where a job's noise is; these calls let a job stop rendering the tiles that have met its target.  A context
 * keeps a set of ACTIVE tiles (all of them after rene_create and rene_reset); rene_render renders the frames it is given on the active tiles
 * only.  The set may only shrink, and under it rene_render must continue where the context stands, so a tile's frames are always the range
 * [F, F + N_t), F the first frame rendered since the context was created or reset (0 in what follows): its image is bit for bit the image of that
 * tile in a context that rendered rene_render(0, N_t) -- every layer, on every kernel family -- and its frame chains hold what the chain rule
 * (frame f in chain f mod 8) gives for those frames.
 *   rene_download / rene_framebuffer keep handing out UN-AVERAGED SUMS, which are now sums over N_t frames, N_t differing from tile to tile:
 *   divide by rene_tile_frames, or take rene_download_mean.  rene_reduce / rene_gather_tiles move those sums unchanged; the caller collects
 *   rene_tile_frames of every shard.
 * Known bias: the stopping rule looks at the same samples it then keeps, so the mean of a tile that was stopped is conditioned on that tile
 * having LOOKED quiet -- a tile whose first frames missed a small light stops with the light missing.  The guards are the first batch (no tile is
 * judged on fewer frames) and `dilate` (a quiet tile beside a noisy one goes on).  Fireflies defeat the rule exactly as they defeat a uniform
 * job rendered to a noise target: one render's tile figure scatters widely where the noise is rare bright samples
 * (rene_resolve_robust below takes them out of the image of an adaptive job too, tile by tile with the tile's own N_t).
 *
 * rene_set_active_tiles: `active` holds one byte per tile of the full tiles_y x tiles_x grid, row-major (n >= tiles_y * tiles_x), non-zero =
 * active; entries of tiles the context does not own are ignored, as rene_download_noise_tiles fills them with zeros.  NULL: every tile active.
 * Waits for the launches issued so far (a launch in flight keeps the set it was launched with), then uploads one bit per owned tile -- a buffer
 * rene_destroy frees and rene_plan_memory does not count.  rene_reset (and rene_tune, which ends in one) makes every tile active again and
 * clears the tiles' frame counts.
 * RENE_ERR_INVALID_ARGUMENT: n too small; a tile that is inactive set active again (until rene_reset); switching tiles off on a context whose
 * frames so far are not one range (a rene_render that did not continue where the one before it ended).
 * RENE_ERR_UNSUPPORTED: a context created with RENE_FLAG_WAVEFRONT (the wavefront integrator is not taught the set), and a frame shard (RENE_SHARD_FRAMES with
 * shard_count > 1: it holds a share of every pixel's frames).
 * While an owned tile is inactive, rene_render(first_frame, n) returns RENE_ERR_INVALID_ARGUMENT unless first_frame == F + the frames rendered so
 * far (rene_stats.frames); with owned tiles of which none is active it returns RENE_OK, launches nothing and counts nothing.  rene_denoise returns
 * RENE_ERR_UNSUPPORTED while owned tiles differ in N_t (its steps take one N): rene_denoise_tiles is the call that filters such an image. */
int rene_set_active_tiles(rene_ctx* ctx, const uint8_t* active, size_t n);
/* N_t, the frames every tile has received, on the full tiles_y x tiles_x grid, row-major (n >= tiles_y * tiles_x entries at dst); 0 for tiles the
 * context does not own.  rene_stats.frames is the N_t of the most-sampled tile; rene_stats.paths counts the paths that were rendered, the sum of
 * N_t n_t over the owned tiles (n_t: the tile's pixels inside the image). */
int rene_tile_frames(rene_ctx* ctx, uint32_t* dst, size_t n);
/* rene_download with every pixel divided by its tile's N_t, on the device: the MEAN image, rows top first, channels 3 or 4 (alpha 0); tiles with
 * N_t == 0 (and tiles the context does not own) are 0.  The division is the correctly rounded IEEE fp32 one: where every tile holds N frames the
 * result is bit for bit rene_download's divided by (float)N.  The first call allocates one layer (16 bytes per pixel) and 4 bytes per tile, which
 * rene_destroy frees and rene_plan_memory does not count. */
int rene_download_mean(rene_ctx* ctx, int layer, int channels, float* dst, size_t dst_floats);
/* rene_estimate_noise on a context whose tiles differ in N_t evaluates every tile with the constants of its own N_t (1 / N, n_c / N, 1 / n_c,
 * 1 / (k - 1)): a tile's record {A_t, B_t, n_t} is bit for bit the one a uniform context gives after rene_render(0, N_t).  Tiles with N_t < 2, or
 * with frames in fewer than two chains, are NOT ESTIMATED: their record is zero (n_pixels == 0) and they enter no figure.  out->n_frames is the
 * largest N_t, out->n_chains the chains that tile's frames fill; the image figures are the same formulas over the tile records.
 *
 * Host only: which tiles of an adaptive job go on.  tiles: the records of the last estimate on the full tiles_x x tiles_y grid (row-major, as
 * rene_download_noise_tiles hands them out); active_in: the tiles active so far, one byte each (NULL: all).  With noisy(t) = active_in[t] and
 * n_t > 0 and sqrt(q_t) > target (q_t by luminance_floor as above): active_out[t] = active_in[t] and n_t > 0 and some tile u within `dilate`
 * steps of t (Chebyshev distance, u == t included) is noisy.  dilate is 0, 1 or 2.  active_out may be active_in.
 * RENE_ERR_INVALID_ARGUMENT: a NULL tiles or active_out, an empty grid, dilate > 2, a floor or target that is not finite and positive. */
int rene_noise_select_tiles(const rene_noise_tile* tiles, const uint8_t* active_in, uint32_t tiles_x, uint32_t tiles_y, float luminance_floor,
                            double target, uint32_t dilate, uint8_t* active_out);

/* ---- firefly-robust resolve (build-defined; ABI v7, added symbols) ------------------------------------------------------------------------------
 * A trimmed mean over the eight frame chains: the chains are eight independent sub-means per pixel, and the ones that stand out are left out of
 * the pixel's mean -- how many, by how unequal the eight are (their Gini coefficient; the adaptive median of means of Buisine et al., EGSR 2021).
 * Opt-in: no other call's output changes.  Per owned pixel inside the image, with C_c the chains' radiance sums, n_c their frame counts (under
 * adaptive sampling they follow from the tile's N_t as rene_estimate_noise derives them), k the chains with n_c > 0; every operation in fp32 and
 * individually rounded in exactly this order -- no fused multiply-add, `/` the correctly rounded IEEE division, denormals kept:
 *   1. for chains with n_c > 0: m_c = C_c / (float)n_c per channel, l_c = (0.2126f m.r + 0.7152f m.g) + 0.0722f m.b;
 *   2. rank r_c = the number of non-empty chains c' with l_c' < l_c, or with l_c' == l_c and c' < c (0-based; 56 comparisons, no sort);
 *   3. tot = sum of l_c in chain order, num = sum in chain order of (float)(2 r_c + 1 - k) l_c,
 *      G = num / ((float)k tot) if tot > 0, else 0 (also for a NaN tot) -- the Gini coefficient of the eight sub-means;
 *   4. t = (gain G) ((float)k 0.5f), j = min((uint)floor(max(t, 0)), max_trim, (k - 1) / 2) (integer division; a NaN t counts as 0);
 *   5. a chain is kept if j <= r_c < k - j; acc = 0, then in chain order acc += C_c for kept chains (chains with n_c == 0 are "kept": adding
 *      their zeros is exact), n_kept = the integer sum of the kept n_c, output mean = acc / (float)n_kept;
 *   6. with k < 2, or on a tile with N_t == 0, the output is the plain mean (0 where there are no frames) and j = 0.
 * Consequence: where j == 0 the pixel is bit for bit rene_download_mean's; with max_trim = 0 the whole image is -- but for the sign of a zero: acc
 * starts from +0, so a pixel whose chains all hold -0.0 comes out +0.0 here and -0.0 there.
 * The estimator is BIASED DARK -- trimming a right-skewed distribution removes more from above than from below -- and converges to the plain
 * mean as frames grow (G falls as the sub-means settle); DESIGN.md section 4c has the error and the energy kept on rene's scenes.  So every owned
 * tile reports what was removed, a 16-byte record reduced in a fixed order without atomics (the same bits from run to run, however the job was
 * cut into calls, and in an unsharded context and the tile shard that owns the tile): sum_lum_plain = sum of lum(S0 / (float)N_t), S0 as
 * rene_download resolves it; sum_lum_robust = sum of lum(output); n_pixels inside the image; n_trimmed = the pixels with j > 0.
 * The accumulation state is read, never written.  Feeding the result to rene_denoise or rene_estimate_noise is not offered. */
typedef struct rene_robust_params {
  uint32_t struct_size;    /* sizeof(rene_robust_params) */
  uint32_t max_trim;       /* 0..3, default 3: at most this many chains are dropped from either end */
  float gain;              /* default 1; finite and > 0: scales G before it is turned into a count */
  uint32_t reserved;
} rene_robust_params;
typedef struct rene_robust_tile {
  float sum_lum_plain;
  float sum_lum_robust;
  uint32_t n_pixels;
  uint32_t n_trimmed;
} rene_robust_tile;
typedef struct rene_robust_summary {
  uint32_t struct_size;    /* sizeof(rene_robust_summary) */
  uint32_t n_tiles;        /* additive: owned tiles */
  uint64_t n_pixels;       /* additive */
  uint64_t n_trimmed;      /* additive */
  double sum_lum_plain;    /* additive; these two summed in fp64 on the host, in tile order */
  double sum_lum_robust;
  double kept_energy;      /* derived: sum_lum_robust / sum_lum_plain, 1 if sum_lum_plain is 0 */
  uint64_t n_frames;       /* the largest N_t */
  uint32_t max_trim;       /* the parameters of the resolve */
  float gain;
} rene_robust_summary;
/* the defaults above; host only */
void rene_robust_params_default(rene_robust_params* out);
/* Resolves the frames accumulated so far (params == NULL: the defaults).  Waits for the launches issued so far, as rene_framebuffer does, runs
 * on the context's stream and returns when *out is filled.  The first call allocates 16 bytes per pixel of the image and 16 bytes per owned
 * tile, which rene_destroy frees and rene_plan_memory does not count.  Every integrator and kernel family is supported -- the call only reads
 * chains.  A RENE_SHARD_TILES shard resolves and reports the tiles it owns; the shards' summaries add.  On a context whose tiles differ in N_t
 * (rene_set_active_tiles) every tile is resolved with the chain counts of its own N_t: its pixels and record are bit for bit those of a uniform
 * context after rene_render(0, N_t).
 * RENE_ERR_INVALID_ARGUMENT: bad struct_size, max_trim > 3, a gain that is not finite and positive, no frames.
 * RENE_ERR_UNSUPPORTED: a frame shard (RENE_SHARD_FRAMES with shard_count > 1: it holds a share of every pixel's frames), and a context whose
 * chains an exchange has consumed (rene_reduce, rene_gather_tiles) until its rene_reset. */
int rene_resolve_robust(rene_ctx* ctx, const rene_robust_params* params, rene_robust_summary* out);
enum { RENE_ROBUST_IMAGE = 0, RENE_ROBUST_TRIM = 1 };
/* The result of the last rene_resolve_robust, rows top first: the robust MEAN radiance as RGB or RGBA (channels 3 or 4, alpha 0), or (float)j
 * per pixel (RENE_ROBUST_TRIM, channels 1).  Tiles the context does not own are 0.  RENE_ERR_INVALID_ARGUMENT: before any resolve since the
 * context was created or reset, a bad `what` or `channels`, dst_floats too small. */
int rene_download_robust(rene_ctx* ctx, int what, int channels, float* dst, size_t dst_floats);
/* The tile records of the last resolve on the full tiles_y x tiles_x grid, row-major (n >= tiles_y * tiles_x records at dst); tiles the context
 * does not own are zero.  RENE_ERR_INVALID_ARGUMENT before any resolve since the context was created or reset. */
int rene_download_robust_tiles(rene_ctx* ctx, rene_robust_tile* dst, size_t n);
/* Host only: the summary of a tile-sharded job from its shards' -- the additive fields summed, n_frames the largest, kept_energy recomputed.
 * RENE_ERR_INVALID_ARGUMENT: n == 0, a bad struct_size, parts whose max_trim or gain differ. */
int rene_robust_combine(const rene_robust_summary* parts, size_t n, rene_robust_summary* out);

/* ---- denoiser `atrous` with firefly rejection: a trimmed prepare (build-defined; ABI v7, added symbols; after the robust resolve, whose params it takes) ---------------------------------------------
 * rene_denoise and rene_denoise_tiles on a scene whose noise is fireflies hand out an image no better than their input: a chain that holds an
 * outlier inflates the pixel's variance, the filter then trusts the pixel less but still spreads it, and what survives is smeared into blotches.
 * The filter reads the frame chains, not rene_resolve_robust's image, so the two do not compose.  These two calls are rene_denoise and
 * rene_denoise_tiles with the robust resolve's decision -- which chains stand out -- taken inside prepare: steps 2 and 3 are computed over the
 * chains that are KEPT.  Opt-in, with a gain of its own (default 0.35: at the robust resolve's 1 most pixels of a 16-frame image are trimmed and
 * quiet scenes come out three times worse than from the plain filter; DESIGN.md section 4c has the study).  rene_denoise itself is unchanged.
 * Per pixel of a valid tile, with k, n_c and N the values of the pixel's tile (of the context, for rene_denoise_robust):
 *   R1. for chains with n_c > 0: m_c = C_c / (float)n_c per channel -- NOT demodulated --, l_c = (0.2126f m.r + 0.7152f m.g) + 0.0722f m.b;
 *   R2. rank r_c = the number of non-empty chains c' with l_c' < l_c, or with l_c' == l_c and c' < c (0-based; 56 comparisons, no sort);
 *   R3. tot = sum of l_c in chain order, num = sum in chain order of (float)(2 r_c + 1 - k) l_c,
 *       G = num / ((float)k tot) if tot > 0, else 0 (also for a NaN tot);
 *   R4. t = (gain G) ((float)k 0.5f), j0 = min((uint)floor(max(t, 0)), max_trim, (k - 1) / 2) (integer division; a NaN t counts as 0)
 *       -- steps 1 - 4 of rene_resolve_robust word for word, every operation in fp32 and individually rounded, no fused multiply-add, `/` the
 *       correctly rounded IEEE division -- then j = min(j0, (k - 2) / 2) (integer division), so that at least TWO non-empty chains are kept: the
 *       variance of step 3' needs them.  Chain c is kept if n_c == 0 or j <= r_c < k - j; h = k - 2 j the non-empty chains kept;
 *   2'. acc = the kept chains' sums added in chain order, starting from C_0 if chain 0 is kept and from +0 otherwise; n_kept = the integer sum
 *       of the kept n_c; d = (acc / n_kept) / den; l = lum(d);
 *   3'. l_c = lum((C_c / n_c) / den) as in step 3; var = sum over kept chains with n_c > 0 of (n_c / n_kept) (l_c - l)^2 / (h - 1);
 *   1, 4, 5. unchanged: the guides are those of the whole pixel, and the radiance out is still col * den * N (N_t in the tiles call) -- the unit of
 *       rene_download, whatever was trimmed.
 * The contract has two parts.  (a) Where j == 0 the pixel's record -- colour, variance, guides -- is bit for bit what rene_denoise
 * (rene_denoise_tiles) prepares: the same constants 1 / N, n_c / N, 1 / n_c, 1 / (k - 1) in the same order; with max_trim = 0 the whole result
 * is therefore bit for bit the existing call's: radiance, variance plane and mean.  Where j > 0 the pixel's 1 / n_kept, n_c / n_kept and
 * 1 / (h - 1) are computed on the device, in fp32 like the rest (2', 3' are not specified to the bit).  (b) j is bit for bit
 * min(rene_resolve_robust's j, (k - 2) / 2) for the same max_trim and gain, on chains whose means are not denormal: the denoiser's units flush
 * denormals, and the contract leaves an implementation free to take R1 - R4 there.  On an even context rene_denoise_tiles_robust equals
 * rene_denoise_robust bit for bit, as the plain calls do.
 * The trimmed estimate is BIASED DARK, as rene_resolve_robust's is, and the filter's own energy loss (see above: it keeps 0.54 - 0.65 of
 * veach-mis) is NOT repaired: these calls remove the blotches, not the loss.
 * Memory: RENE_DENOISE_BYTES_PER_PIXEL as for rene_denoise, and 4 bytes per pixel more for the trim words, allocated by the first of these two
 * calls, freed by rene_destroy and not counted by rene_plan_memory; the tiles call's table is 108 bytes per distinct N_t and 4 bytes per tile.
 * Validation is the union of the parents': RENE_ERR_INVALID_ARGUMENT for bad denoise params, a bad robust struct_size, max_trim > 3, a gain that
 * is not finite and positive, frames in fewer than two chains (the tiles call: no valid owned tile), a chain with more than 2^32 - 1 frames;
 * RENE_ERR_UNSUPPORTED for shard_count > 1 (only the plain filter is offered for tile shards), a context whose chains an exchange has consumed and -- rene_denoise_robust only -- owned tiles that
 * differ in their frame counts.  A refusal leaves the context usable and the previous result downloadable. */
/* max_trim 3, gain 0.35; host only */
void rene_denoise_robust_params_default(rene_robust_params* out);
int rene_denoise_robust(rene_ctx* ctx, const rene_denoise_params* params, const rene_robust_params* robust);        /* NULL: the defaults */
int rene_denoise_tiles_robust(rene_ctx* ctx, const rene_denoise_params* params, const rene_robust_params* robust);

/* ---- denoiser hand-off: feature tensors from the chains (build-defined; ABI v7, added symbols) ---------------------------------------------------
 * rene averages its radiance, normal and albedo layers and hands three packed float3 images to OIDN or OptiX (rene/src/main.rs:1617-1647).  On
 * this build the consumers live on the device -- OIDN's HIP backend takes device pointers and strided images, a network takes an NCHW tensor --
 * so the hand-off is one call that writes, on the device and in one pass over the frame chains, a tensor of MEANS in the layout and precision
 * the consumer wants; the chains add what rene could not give: two independent half-images, a per-pixel variance of the mean, the sample count.
 * Opt-in: no other call's output changes.  It is correct on adaptive jobs (every pixel over its own tile's N_t) and on tile shards.
 *
 * Layout: the channels of the mask in bit order; RENE_FEATURES_CHW is [C][H][W], RENE_FEATURES_HWC is [H][W][C], rows top first, tightly packed.
 * With HWC and COLOR | ALBEDO | NORMAL (the default) a consumer of float3 images reads three of them at byte offsets 0, 12 and 24 with a pixel
 * stride of 36 bytes; in CHW they are three planes each.
 *
 * Arithmetic, per owned pixel inside the image, every operation in fp32 and individually rounded in exactly this order -- no fused multiply-add,
 * `/` the correctly rounded IEEE division, denormals kept.  C_c, n_c and k as for the robust resolve above (under adaptive sampling the n_c follow from
 * the tile's N_t in the same way), N = N_t, lum(v) = (0.2126f v.r + 0.7152f v.g) + 0.0722f v.b:
 *   COLOR    = S0 / (float)N, S0 = ((C_0 + C_1) + ...) + C_7;
 *   ALBEDO, NORMAL = the resolved layer sums / (float)N -- with COLOR bit for bit rene_download_mean of layers 2, 1 and 0;
 *   HALF_A   = (((C_0 + C_2) + C_4) + C_6) / (float)(n_0 + n_2 + n_4 + n_6), HALF_B the same over the chains 1, 3, 5, 7; a half without frames is 0;
 *   VARIANCE: for chains with n_c > 0, m_c = C_c / (float)n_c and l_c = lum(m_c); l = lum(COLOR); v = 0, then in chain order t = l_c - l,
 *              v = v + ((float)n_c / (float)N) (t t); VARIANCE = v / (float)(k - 1), 0 when k < 2;
 *   FRAMES   = (float)N;
 *   a tile with N_t == 0 is all zeros.
 * RENE_FEATURES_F16: the fp32 value clamped to +-65504, then converted with round-to-nearest-even, subnormals kept; a NaN stays a NaN. */
enum { RENE_FEATURE_COLOR = 1u << 0,    /* 3: mean radiance */
       RENE_FEATURE_ALBEDO = 1u << 1,   /* 3: mean first-hit albedo */
       RENE_FEATURE_NORMAL = 1u << 2,   /* 3: mean first-hit normal, not renormalised */
       RENE_FEATURE_VARIANCE = 1u << 3, /* 1: variance of the mean's luminance, from the chains */
       RENE_FEATURE_HALF_A = 1u << 4,   /* 3: mean radiance over the even chains 0, 2, 4, 6 */
       RENE_FEATURE_HALF_B = 1u << 5,   /* 3: mean radiance over the odd chains 1, 3, 5, 7 */
       RENE_FEATURE_FRAMES = 1u << 6 }; /* 1: (float)N_t */
enum { RENE_FEATURES_F32 = 0, RENE_FEATURES_F16 = 1 };
enum { RENE_FEATURES_CHW = 0, RENE_FEATURES_HWC = 1 };
typedef struct rene_feature_params {
  uint32_t struct_size;    /* sizeof(rene_feature_params) */
  uint32_t features;       /* RENE_FEATURE_* mask, not empty */
  uint32_t format;         /* RENE_FEATURES_F32 or _F16 */
  uint32_t layout;         /* RENE_FEATURES_CHW or _HWC */
} rene_feature_params;
/* COLOR | ALBEDO | NORMAL, F32, HWC -- rene's own hand-off; host only */
void rene_feature_params_default(rene_feature_params* out);
/* the channels a mask selects; 0 for an empty mask or one with unknown bits; host only */
uint32_t rene_feature_channels(uint32_t features);
/* Exports the frames accumulated so far (params == NULL: the defaults).  Waits for the launches issued so far, runs on the context's stream and
 * returns when the result is there; the accumulation state is read, never written.
 * device_dst != NULL: a caller-owned device buffer (a tensor's data pointer, say) of dst_bytes >= C * H * W * element size.  It is checked before
 * anything is launched: device memory of the context's device, aligned to the element, with dst_bytes from the pointer to the end of its
 * allocation -- a host pointer never reaches a kernel.
 * device_dst == NULL: a buffer of the library's own, allocated or regrown on demand and zeroed on the context's stream when it is (and when the
 * mask, format or layout differ from the export before), freed by rene_destroy and not counted by rene_plan_memory; dst_bytes is ignored.
 * Only the pixels of owned tiles inside the image are written: the tiles of other shards are left as they are, so the RENE_SHARD_TILES shards of
 * one device can fill one caller-owned tensor.  Every integrator and kernel family is supported, RENE_FLAG_NO_AOV (the guides are 0) and a
 * context without frames (all zeros) included.
 * RENE_ERR_INVALID_ARGUMENT: bad struct_size, an empty mask or unknown bits, a bad format or layout, a bad destination -- nothing is launched.
 * RENE_ERR_UNSUPPORTED: a frame shard, and a context whose chains an exchange has consumed until its rene_reset (as for the robust resolve). */
int rene_export_features(rene_ctx* ctx, const rene_feature_params* params, void* device_dst, size_t dst_bytes);
/* The library-owned result of the last export with device_dst == NULL: its device pointer (valid until the next such export, rene_reset or
 * rene_destroy) and size in bytes, or a copy in host memory (dst_bytes >= that size).  RENE_ERR_INVALID_ARGUMENT before any such export since the
 * context was created or reset. */
int rene_features_buffer(rene_ctx* ctx, void** device_ptr, size_t* n_bytes);
int rene_download_features(rene_ctx* ctx, void* dst, size_t dst_bytes);

/* ---- output transform on the device: 8-bit images from a context (build-defined; ABI v7, added symbols) ----------------------------------------
 * rene's path ends in average + to_rgb8 / to_aov (rene/src/main.rs:1758-1810) on the host, after three float layers have come back from the GPU.
 * rene_output_8bit is that stage on the device: one call turns an image the context can hand out into tightly packed 8-bit pixels, in a buffer of
 * the library's or in the caller's (a uint8 tensor's data pointer, say), and only 3 or 4 bytes per pixel ever cross PCIe.  Opt-in: no other call's
 * output changes.  The bytes are BIT FOR BIT those of the host functions at the end of this header:
 *   source                       the bytes equal                                                                         transform
 *   RENE_OUTPUT_RADIANCE         rene_to_rgb8 of what rene_download_mean hands out for layer 0, with n_samples 1          sRGB
 *                                (on an even context of N frames: rene_to_rgb8 of rene_download's sums with n_samples N)
 *   RENE_OUTPUT_NORMAL           rene_to_aov8, is_normal 1, of rene_download_mean's layer 1, n_samples 1                 AOV, normal
 *   RENE_OUTPUT_ALBEDO           rene_to_aov8, is_normal 0, of rene_download_mean's layer 2, n_samples 1                 AOV
 *   RENE_OUTPUT_DENOISED         rene_to_rgb8 of rene_download_denoised's RENE_DENOISED_RADIANCE with n_samples N,       sRGB
 *                                N = rene_stats.frames; refused while owned tiles differ in their frame counts
 *   RENE_OUTPUT_DENOISED_MEAN    rene_to_rgb8 of rene_download_denoised's RENE_DENOISED_MEAN, n_samples 1, the invalid    sRGB
 *                                tiles' unfiltered means included: the source for adaptive jobs
 *   RENE_OUTPUT_ROBUST           rene_to_rgb8 of rene_download_robust's RENE_ROBUST_IMAGE, n_samples 1                   sRGB
 * The mean is s / (float)N_t per channel, the correctly rounded IEEE division of rene_download_mean (N_t == 0: 0).  The AOV transforms are IEEE
 * arithmetic without contraction.  The sRGB transform does not evaluate a pow on the device: as a map float -> byte, rene_to_rgb8 with n_samples 1
 * is monotone with exactly 255 steps (NaN, negatives and -0.0 give 0, +infinity 255), so the byte of v is the number of thresholds T[k] <= v,
 * T[k] the smallest float the host function maps to k + 1.  rene_output_thresholds hands the table out; it is derived from rene_to_rgb8 itself,
 * by bisection over bit patterns, once per process, and the device looks the byte up in it.
 * Formats: RENE_OUTPUT_RGB8 is [H][W][3], RENE_OUTPUT_RGBA8 is [H][W][4] with alpha 255; rows top first, tightly packed.
 * The call waits for the launches issued so far, runs on the context's stream and returns when the bytes are there; it reads the image and writes
 * nothing of the accumulation state.  Every integrator and kernel family is supported, and adaptive contexts (every pixel over its own tile's N_t).
 * On a RENE_SHARD_TILES shard -- RADIANCE, NORMAL, ALBEDO and ROBUST -- only the pixels of owned tiles inside the image are written and every other
 * byte of the destination is left as it was, so the tile shards of one device can fill one caller-owned buffer.
 * device_dst != NULL: a caller-owned device buffer of dst_bytes >= H * W * 3 (or 4), checked before anything is launched as rene_export_features
 * checks its destination: device memory of the context's device, 4-byte aligned, with dst_bytes from the pointer to the end of its allocation -- a
 * host pointer never reaches a kernel.
 * device_dst == NULL: a buffer of the library's own, allocated or regrown on demand and zeroed on the context's stream when it is (and when the
 * format differs from the call before), freed by rene_destroy and not counted by rene_plan_memory; dst_bytes is ignored.
 * RENE_ERR_INVALID_ARGUMENT: bad struct_size, source or format, a bad destination; DENOISED, DENOISED_MEAN or ROBUST before a valid result of their
 * own call (rene_denoise and its kin, rene_resolve_robust) since the context was created or reset -- nothing is launched.
 * RENE_ERR_UNSUPPORTED: a frame shard, and a context whose chains an exchange has consumed until its rene_reset (as for the robust resolve; the
 * root's image after rene_gather_tiles is not offered); DENOISED on uneven tiles; DENOISED and DENOISED_MEAN on a context with shard_count > 1. */
enum { RENE_OUTPUT_RADIANCE = 0, RENE_OUTPUT_NORMAL = 1, RENE_OUTPUT_ALBEDO = 2, RENE_OUTPUT_DENOISED = 3, RENE_OUTPUT_DENOISED_MEAN = 4,
       RENE_OUTPUT_ROBUST = 5 };
enum { RENE_OUTPUT_RGB8 = 0, RENE_OUTPUT_RGBA8 = 1 };
enum { RENE_OUTPUT_SRGB = 0, RENE_OUTPUT_AOV = 1, RENE_OUTPUT_AOV_NORMAL = 2 };  /* the transforms, for rene_output_probe */
typedef struct rene_output_params {
  uint32_t struct_size;    /* sizeof(rene_output_params) */
  uint32_t source;         /* RENE_OUTPUT_RADIANCE .. RENE_OUTPUT_ROBUST */
  uint32_t format;         /* RENE_OUTPUT_RGB8 or _RGBA8 */
  uint32_t reserved;
} rene_output_params;
/* RADIANCE, RGB8; host only */
void rene_output_params_default(rene_output_params* out);
int rene_output_8bit(rene_ctx* ctx, const rene_output_params* params, void* device_dst, size_t dst_bytes);
/* The library-owned result of the last rene_output_8bit with device_dst == NULL: its device pointer (valid until the next such call, rene_reset or
 * rene_destroy) and size in bytes, or a copy in host memory (dst_bytes >= that size).  RENE_ERR_INVALID_ARGUMENT before any such call since the
 * context was created or reset. */
int rene_output_buffer(rene_ctx* ctx, void** device_ptr, size_t* n_bytes);
int rene_download_output(rene_ctx* ctx, uint8_t* dst, size_t dst_bytes);
/* The 255 thresholds of the sRGB transform, strictly increasing, the last at most 1; host only, no GPU needed. */
void rene_output_thresholds(float out[255]);
/* Probe of the device transform: out[i] = the byte of the MEAN v[i] under `transform` (RENE_OUTPUT_SRGB, _AOV, _AOV_NORMAL), computed by the
 * per-channel device function the kernel of rene_output_8bit uses.  Host pointers. */
int rene_output_probe(int device, int transform, size_t n, const float* v, uint8_t* out);

/* ---- tone-mapped output on the device: exposure and a tone curve ahead of the sRGB byte (build-defined; ABI v7, added symbols) ------------------
 * rene_output_8bit is rene's average + to_rgb8 and nothing else: every radiance above 1 becomes byte 255.  rene_output_tonemapped is the same
 * stage with an exposure factor and a tone curve between the mean and its byte, and rene_luminance_histogram is the image-wide statistic from which
 * an automatic exposure is chosen.  Opt-in: no other call's output changes.  Everything is specified operation by operation, so the bytes and the
 * counts are BIT FOR BIT those of the host functions rene_tonemap_rgb8 and rene_luminance_histogram_host below (tests/tonemap_reference.py restates
 * them in numpy).  Every fp32 operation below is rounded once; there is no fused multiply-add and no transcendental.
 *
 * Per pixel.  The mean v is rene_output_8bit's: s / (float)N_t per channel, N_t == 0 giving 0.  lum3(r, g, b) = (0.2126f r + 0.7152f g) + 0.0722f b.
 * fmaxf / fminf return the other argument where one is a NaN.
 *   1. exposure   e_c = v_c * scale                                            (scale: a finite fp32 > 0)
 *   2. operator   RENE_TONEMAP_CLAMP      c_c = e_c
 *                 RENE_TONEMAP_REINHARD   extended Reinhard on the luminance, so that the hue is kept:
 *                                         l = fminf(fmaxf(lum3(e), 0.0f), FLT_MAX);  q = l / w2;  a = 1.0f + q;  b = 1.0f + l;  f = a / b;  c_c = e_c * f
 *                                         w2 = white * white, rounded to fp32 once on the host (white: a finite fp32 > 0, 4 by default: the
 *                                         exposed luminance that maps to 1).  The lower clamp keeps a pixel whose luminance is negative or a
 *                                         NaN as it is (f = 1), so that a negative channel cannot turn positive.
 *                 RENE_TONEMAP_ACES       Narkowicz's fit of the ACES curve, per channel:
 *                                         x = fminf(fmaxf(e_c, 0.0f), 16777216.0f);  n = x * (2.51f * x + 0.03f);  d = x * (2.43f * x + 0.59f) + 0.14f;
 *                                         c_c = n / d
 *   3. byte       the byte of c_c under the sRGB threshold table of rene_output_thresholds: rene_to_rgb8 of c_c with n_samples 1.
 * So RENE_TONEMAP_CLAMP with scale 1.0f gives the bytes of rene_output_8bit; a +infinity mean gives 255, a NaN or negative mean 0 under every
 * operator; a tile with N_t == 0 is 0.
 *
 * The luminance histogram, over the pixels the call would write (inside the image; on a RENE_SHARD_TILES shard the owned tiles only): l = lum3(v)
 * of the UN-exposed mean.  A pixel with !(l > 0) -- zero, negative, NaN -- is counted in n_dark.  Every other pixel is counted in one of 256 bins
 * taken from the float's bit pattern, eight per octave from 2^-20 to 2^12: bin = clamp((int)(bits(l) >> 20) - 856, 0, 255) -- bin b holds
 * 2^(b / 8 - 20) (1 + (b % 8) / 8) and up, exclusive of the next; denormals and everything below 2^-20 fall in bin 0, everything from 2^12 up and
 * +infinity in bin 255.  Counts are sums of ones in uint32: the histogram of an unsharded context is the element-wise sum of its tile shards'
 * histograms, exactly (rene_luminance_combine).  n_pixels == n_dark + the sum of the counts.
 *
 * Statistics and exposure from a histogram: host only, unsigned 64-bit integers.
 *   n_lit          = sum of count_b
 *   mean_bin_x256  = (sum of count_b * (2 b + 1)) * 128 / n_lit, floor division: 256 times the mean bin, every pixel at its bin's centre (0: n_lit == 0)
 *   percentile bin   of a per-mille p (<= 1000): the smallest b whose cumulative count reaches (n_lit * p + 999) / 1000  (-1: n_lit == 0)
 *   e8             = key_e8 + 160 - ((mean_bin_x256 + 128) >> 8), held to RENE_EXPOSURE_E8_MIN .. _MAX: the automatic exposure in eighth-stops,
 *                    which moves the mean log2 luminance onto key_e8 / 8.  RENE_EXPOSURE_KEY_E8 = -20 is 2^-2.5, about 0.18.  n_lit == 0: 0.
 *   rene_exposure_scale(e8) = M[e8 mod 8] * 2^floor(e8 / 8) (mod and floor toward minus infinity; e8 held to RENE_EXPOSURE_E8_MIN .. _MAX, where
 *                    the result is a normal float): M = RENE_EXPOSURE_MANTISSAS, eight fp32 literals equal to (float)2^(k / 8); the power of two
 *                    is applied with ldexpf, which is exact.  No exp2 of a fraction is evaluated anywhere: the scale is the same on every machine. */
enum { RENE_TONEMAP_CLAMP = 0, RENE_TONEMAP_REINHARD = 1, RENE_TONEMAP_ACES = 2 };
#define RENE_EXPOSURE_KEY_E8 (-20)
#define RENE_EXPOSURE_E8_MIN (-960)
#define RENE_EXPOSURE_E8_MAX 960
#define RENE_EXPOSURE_MANTISSAS { 1.0f, 1.0905077f, 1.1892071f, 1.2968396f, 1.4142135f, 1.5422108f, 1.6817929f, 1.8340081f }
#define RENE_LUMINANCE_BINS 256
typedef struct rene_tonemap_params {
  uint32_t struct_size;    /* sizeof(rene_tonemap_params) */
  uint32_t source;         /* RENE_OUTPUT_RADIANCE, _DENOISED, _DENOISED_MEAN or _ROBUST: the sRGB sources */
  uint32_t format;         /* RENE_OUTPUT_RGB8 or _RGBA8 */
  uint32_t op;             /* RENE_TONEMAP_CLAMP, _REINHARD or _ACES */
  float scale;             /* the exposure's factor, finite and > 0 (rene_exposure_scale makes one from eighth-stops) */
  float white;             /* RENE_TONEMAP_REINHARD: finite and > 0; checked under every operator */
  uint32_t reserved[2];
} rene_tonemap_params;
/* RADIANCE, RGB8, CLAMP, scale 1, white 4; host only */
void rene_tonemap_params_default(rene_tonemap_params* out);
/* rene_output_8bit with exposure and a tone curve.  The destination (device_dst / dst_bytes, the library-owned buffer behind rene_output_buffer and
 * rene_download_output when device_dst == NULL), the refusals, the behaviour on tile shards and the RENE_DEBUG line are rene_output_8bit's.
 * RENE_ERR_INVALID_ARGUMENT in addition, before anything is launched: a source of RENE_OUTPUT_NORMAL or _ALBEDO (tone curves are for radiance), an
 * unknown operator, a scale or white that is not finite and > 0. */
int rene_output_tonemapped(rene_ctx* ctx, const rene_tonemap_params* params, void* device_dst, size_t dst_bytes);
typedef struct rene_luminance_stats {
  uint32_t struct_size;                    /* sizeof(rene_luminance_stats) */
  uint32_t counts[RENE_LUMINANCE_BINS];
  uint32_t n_dark;                         /* pixels with !(l > 0) */
  uint32_t n_pixels;                       /* the pixels looked at: n_dark + the sum of counts */
} rene_luminance_stats;
/* The luminance histogram of `source` (those of rene_output_tonemapped, with its refusals), counted on the device; 257 integers come back. */
int rene_luminance_histogram(rene_ctx* ctx, uint32_t source, rene_luminance_stats* out);
/* Host only, no GPU needed.  rene_luminance_combine: out = the element-wise sum of n histograms (tile shards of one image; out may be parts[0]);
 * RENE_ERR_INVALID_ARGUMENT on a bad struct_size or a sum beyond uint32.  The three statistics and the scale are the integers and the float
 * specified above (a NULL or mismatched stats: 0, -1, 0). */
int rene_luminance_combine(const rene_luminance_stats* parts, size_t n, rene_luminance_stats* out);
uint32_t rene_luminance_mean_bin_x256(const rene_luminance_stats* stats);
int rene_luminance_percentile_bin(const rene_luminance_stats* stats, uint32_t per_mille);
int rene_auto_exposure_e8(const rene_luminance_stats* stats, int key_e8);
float rene_exposure_scale(int e8);
/* The host forms of the two device passes, the same arithmetic: means is [n_pixels][channels] fp32 (channels 3 or 4; the first three are read),
 * out [n_pixels][3] bytes / the histogram with n_pixels filled in.  RENE_ERR_INVALID_ARGUMENT: NULL pointers, channels, an unknown operator, a
 * scale or white that is not finite and > 0, more than 2^32 - 1 pixels for the histogram. */
int rene_tonemap_rgb8(const float* means, size_t n_pixels, int channels, uint32_t op, float scale, float white, uint8_t* out);
int rene_luminance_histogram_host(const float* means, size_t n_pixels, int channels, rene_luminance_stats* out);
/* Probe of the device's per-pixel function: out[3 i ..] = the bytes of the MEAN rgb[3 i ..] under `op`, `scale` and `white`, computed by the
 * function the kernel of rene_output_tonemapped uses, one lane per pixel.  Host pointers. */
int rene_tonemap_probe(int device, uint32_t op, float scale, float white, size_t n, const float* rgb, uint8_t* out);

/* ---- the geometry pass: first-hit depth, position, coverage and id mattes ----------------------------------------------------------------------
 * Beside radiance, first-hit normal and first-hit albedo a compositor wants depth, world position, coverage and anti-aliased id mattes.
 * rene_gbuffer computes them in one device pass over the primary rays of frames first_frame .. first_frame + n_frames - 1 -- the rays those
 * frames' paths start with: the same seeds (rene_frame_seeds of the context's master seed), the same jitter, the same camera -- and one
 * closest-hit query each (tmin 0.001, tmax 100000, the render kernels').  Nothing is shaded and nothing bounces.  The pass reads nothing of the
 * accumulation state and changes nothing of it: it may be called before, between and after rene_render calls, on tile shards (every shard
 * fills the pixels of its tiles; the rest of its record array is zero) and on adaptive contexts (the frames are the caller's: the mask of
 * active tiles plays no part).  On a volpath scene the pass reports the closest hit of the main structure WHATEVER its material: the
 * None-material boundary of a medium is a hit, with its instance's ids.
 *
 * Per sample: t is the hit distance along the normalised direction d, the position is o + t d per component as a rounded multiply followed by a
 * rounded add (no fused multiply-add).  Per pixel, in frame order: depth_sum and position_sum are plain fp32 running sums over the hitting
 * samples, depth_min their fminf starting at +infinity.  coverage = hits / n, mean depth = depth_sum / hits.
 * The id of a hitting sample is its instance (RENE_GBUFFER_ID_INSTANCE: the `instance` word of rene_trace), that instance's material index
 * (_MATERIAL) or its `primitive` word (_PRIMITIVE); a miss has none.  Four slots are filled by a streaming rule: the id is in a slot -> its
 * count + 1; else a slot is free -> the lowest free slot takes it with count 1; else other + 1 (nothing is evicted).  After the last frame
 * the slots are ordered by count descending, ties by id ascending; an unused slot holds id 0xffffffff, count 0.  count / n of an id is its
 * anti-aliased matte. */
#define RENE_GBUFFER_ID_INSTANCE 0u
#define RENE_GBUFFER_ID_MATERIAL 1u
#define RENE_GBUFFER_ID_PRIMITIVE 2u
#define RENE_GBUFFER_MAX_FRAMES 65536u
typedef struct rene_gbuffer_params {
  uint32_t struct_size;  /* sizeof(rene_gbuffer_params) */
  uint32_t first_frame;
  uint32_t n_frames;     /* 1 .. RENE_GBUFFER_MAX_FRAMES */
  uint32_t id_source;    /* RENE_GBUFFER_ID_* */
  uint32_t flags;        /* reserved: 0 */
} rene_gbuffer_params;
typedef struct rene_gbuffer_pixel {  /* 64 bytes; the array is pixel-major [H][W], rows top first */
  float depth_sum;
  float depth_min;       /* +infinity where nothing hit */
  uint32_t hits;
  uint32_t n;            /* n_frames for every pixel of a tile the context owns, 0 elsewhere (the all-zero record) */
  float position_sum[3];
  uint32_t other;        /* hitting samples whose id found no slot */
  uint32_t id[4];
  uint32_t count[4];
} rene_gbuffer_pixel;
typedef struct rene_primary_hit {    /* 32 bytes: one sample */
  float d[3];            /* the primary ray's direction (its origin is the translation column of camera_to_world) */
  float t;               /* -1: a miss (u, v, instance, primitive are 0 then) */
  float u, v;
  uint32_t instance, primitive;
} rene_primary_hit;
/* frames 0 .. 15, instance ids */
void rene_gbuffer_params_default(rene_gbuffer_params* out);
/* width x height x sizeof(rene_gbuffer_pixel); host only */
size_t rene_gbuffer_bytes(uint32_t width, uint32_t height);
/* The pass, into device_dst (device memory of the context's device, 16-byte aligned, at least rene_gbuffer_bytes; all of those bytes are written:
 * zeroed, then the owned pixels' records) or, with device_dst == NULL, into a buffer the library owns (allocated by the first such call, outside
 * rene_plan_memory's figures, like the output buffer).  Ordered on the context's stream like rene_output_8bit.  params == NULL: the defaults.
 * RENE_ERR_INVALID_ARGUMENT: a NULL context, a struct_size that is not this build's, n_frames outside 1 .. 65536, an unknown id_source, flags
 * other than 0, a destination that is too small, misaligned or not device memory of the context's device. */
int rene_gbuffer(rene_ctx* ctx, const rene_gbuffer_params* params, void* device_dst, size_t dst_bytes);
/* The library-owned result of the last rene_gbuffer with device_dst == NULL (valid until the next such call or rene_destroy), and its download. */
int rene_gbuffer_buffer(rene_ctx* ctx, void** device_ptr, size_t* n_bytes);
int rene_download_gbuffer(rene_ctx* ctx, void* dst, size_t dst_bytes);
/* Probe: every sample the pass aggregates -- the same ray, the same query, the same device function -- as [n_frames][H][W] records in host memory
 * (n = n_frames x width x height records, at most 2^24).  Samples of pixels in tiles the context does not own are all zero. */
int rene_primary_hits(rene_ctx* ctx, uint32_t first_frame, uint32_t n_frames, rene_primary_hit* host_dst, size_t n);

/* ---- the occlusion pass: ambient occlusion and bent normals from the first hit (build-defined; ABI v7, added symbols) -----------------------------
 * An ambient-occlusion layer, its bent normal (the mean unoccluded direction) and with them a sky-visibility figure, from the primary rays of
 * frames first_frame .. first_frame + n_frames - 1: the seeds, the jitter, the camera and the closest-hit query of the geometry pass above.
 * Opt-in: no other call's output changes.  Like the geometry pass it reads nothing of the accumulation state and changes nothing of it, runs on
 * the context's stream, on tile shards and on adaptive contexts (the mask of active tiles plays no part).
 *
 * The sample of pixel (px, py) under frame seed s:
 *   1. rng = PCG32si::new((py W + px) ^ s); two f32 draws are the jitter; the primary ray and its closest hit (tmin 0.001, tmax 100000, the main
 *      structure).  A miss contributes nothing.
 *   2. The closest-hit shader's surface: its position, and its normal as the shader leaves it.  n = normalize(normal), negated when
 *      dot(normal, d) > 0: it faces the viewer.  Where a component of n is not finite the sample counts in `hits` and casts no rays.
 *   3. For k = 0 .. rays - 1, the same generator going on: the Matte bounce's cosine-distributed direction (math.rs:45-56: draws r1, then r2)
 *      carried into the frame of n (onb.rs), w; ONE any-hit query of the main structure from the position along w with tmin 0.001 and
 *      tmax = radius.  Occluded or not, whatever was hit: the None-material boundary of a medium occludes, as it is a hit for the geometry pass.
 *   4. Per pixel, in frame order and within a frame in k order: hits + 1 per hitting sample; per ray cast rays + 1, occluded + verdict, and for
 *      the unoccluded rays only bent_sum + w, a plain fp32 add per component.
 * ao = 1 - occluded / rays (rays == 0: 1) is the ambient occlusion -- with a radius beyond the scene's extent, the visibility of the sky;
 * bent = bent_sum / |bent_sum| (0 where bent_sum is 0) the bent normal. */
#define RENE_OCCLUSION_MAX_RAYS 64u
#define RENE_OCCLUSION_MAX_FRAMES 65536u
#define RENE_OCCLUSION_MISS 0u      /* rene_occlusion_sample.state: the primary ray hit nothing (the whole record is zero) */
#define RENE_OCCLUSION_OPEN 1u      /* the ray is unoccluded */
#define RENE_OCCLUSION_OCCLUDED 2u
#define RENE_OCCLUSION_NO_RAY 3u    /* a hit that cast nothing (p and n hold; r1, w, r2 are zero) */
typedef struct rene_occlusion_params {
  uint32_t struct_size;  /* sizeof(rene_occlusion_params) */
  uint32_t first_frame;
  uint32_t n_frames;     /* 1 .. RENE_OCCLUSION_MAX_FRAMES */
  uint32_t rays;         /* per hitting sample, 1 .. RENE_OCCLUSION_MAX_RAYS */
  float radius;          /* the occlusion rays' tmax in world units: finite, > 0.001, <= 100000 */
  uint32_t flags;        /* reserved: 0 */
} rene_occlusion_params;
typedef struct rene_occlusion_pixel {  /* 32 bytes; the array is pixel-major [H][W], rows top first */
  uint32_t hits;         /* samples whose primary ray hit */
  uint32_t rays;         /* occlusion rays cast */
  uint32_t occluded;     /* ... that hit something within the radius */
  uint32_t n;            /* n_frames for every pixel of a tile the context owns, 0 elsewhere (the all-zero record) */
  float bent_sum[3];     /* the sum of the unoccluded rays' directions */
  uint32_t reserved;     /* 0 */
} rene_occlusion_pixel;
typedef struct rene_occlusion_sample {  /* 48 bytes: one occlusion ray (or the sample that cast none) */
  float p[3];            /* where the ray starts: the first hit's position */
  uint32_t state;        /* RENE_OCCLUSION_MISS, _OPEN, _OCCLUDED, _NO_RAY */
  float n[3];            /* the unit normal facing the viewer */
  float r1;
  float w[3];            /* the ray's direction */
  float r2;
} rene_occlusion_sample;
/* frames 0 .. 15, one ray per sample, radius 1 */
void rene_occlusion_params_default(rene_occlusion_params* out);
/* width x height x sizeof(rene_occlusion_pixel); host only */
size_t rene_occlusion_bytes(uint32_t width, uint32_t height);
/* The pass, into device_dst (device memory of the context's device, 16-byte aligned, at least rene_occlusion_bytes; all of those bytes are
 * written: zeroed, then the owned pixels' records) or, with device_dst == NULL, into a buffer the library owns (allocated by the first such
 * call, outside rene_plan_memory's figures, like the geometry pass's).  params == NULL: the defaults.
 * RENE_ERR_INVALID_ARGUMENT, before anything is launched: a NULL context, a struct_size that is not this build's, n_frames outside 1 .. 65536,
 * rays outside 1 .. 64, a radius that is not finite, not above 0.001 or above 100000, flags other than 0, a destination that is too small,
 * misaligned or not device memory of the context's device. */
int rene_occlusion(rene_ctx* ctx, const rene_occlusion_params* params, void* device_dst, size_t dst_bytes);
/* The library-owned result of the last rene_occlusion with device_dst == NULL (valid until the next such call or rene_destroy), and its download. */
int rene_occlusion_buffer(rene_ctx* ctx, void** device_ptr, size_t* n_bytes);
int rene_download_occlusion(rene_ctx* ctx, void* dst, size_t dst_bytes);
/* Probe: every ray the pass aggregates -- the same device functions -- as [n_frames][rays][H][W] records in host memory (n = n_frames x rays x
 * width x height records, at most 2^22).  The records of pixels in tiles the context does not own are all zero.  params as above. */
int rene_occlusion_samples(rene_ctx* ctx, const rene_occlusion_params* params, rene_occlusion_sample* host_dst, size_t n);

/* ---- the direct-light pass: the path estimator's first two steps, per pixel (build-defined; ABI v7, added symbols) ---------------------------------
 * The direct light on its own, and with it the indirect light as beauty - direct.  rene's estimator has no separate direct term: one light / BSDF
 * mixture ray per bounce, whose emission is added at the NEXT iteration (lib.rs:225-227, 274-324).  The pass is therefore a PREFIX of that
 * estimator, replayed from the seeds of frames first_frame .. first_frame + n_frames - 1: all of iteration 0, then iteration 1's closest-hit
 * query and its one emission-or-background add.  It draws the random numbers the job's frames draw, so beauty - direct is the indirect light of
 * the same samples.  Path-integrator scenes only: a context whose scene selects volpath returns RENE_ERR_UNSUPPORTED.  Opt-in: no other call's
 * output changes.  Like the geometry pass it reads nothing of the accumulation state and changes nothing of it, runs on the context's stream,
 * on tile shards and on adaptive contexts (the mask of active tiles plays no part); rene_reset does not invalidate the result.
 *
 * The sample of pixel (px, py) under frame seed s:
 *   1. rng = PCG32si::new((py W + px) ^ s), whose first two f32 draws are the jitter; fw = PCG32si::new(s).  The primary ray and its closest hit
 *      in the main structure (tmin 0.001, tmax 100000), as the geometry pass traces it.
 *   2. A miss: seen += miss colour(rd) (the background colour times its texture; 0 without a background).  The sample ends (state MISS).
 *   3. A hit: the closest-hit shader's surface; wo = -normalize(rd), normal = normalize(sf.normal); the BSDF as the render kernels build it.
 *      If the instance emits: seen += e where dot(wo, normal) > 0 (else + 0).
 *   4. For every distant light, in table order: wi = normalize((position + dir) - position); ONE any-hit query of the main structure from the
 *      position along wi (tmin 0.001, tmax 1e5); unoccluded: distant += f(wo, wi) |dot(wi, normal)| L.
 *   5. The mixture (lib.rs:274-337).  With emit_object_len > 0 and a diffuse lobe in the BSDF: the coin from fw; > 0.5 (state LIGHT): the object
 *      fw.next_u32() % emit_object_len, the point from the emitter's sampler on fw, wi towards it, pdf = bsdf_pdf(wi, normal) (quirk Q1),
 *      f = f(wo, wi); else (state BSDF) the BSDF's sample on rng.  Then the closest-hit query of the EMITTER structure along wi for pdf_l,
 *      T = f |dot(normal, wi)|, pdf = 0.5 pdf + 0.5 pdf_l / emit_object_len; pdf < 1e-5: the sample ends (ENDED_PDF), else T /= pdf.
 *      Without emitters or without a diffuse lobe (state PLAIN): the BSDF's sample s on rng; s.pdf < 1e-5: the sample ends (ENDED_PDF), else
 *      T = s.f (|dot(normal, s.wi)| / s.pdf).
 *   6. T == 0 in all three components: the sample ends (ENDED_ZERO; lib.rs:340-342).
 *   7. ONE closest-hit query of the main structure from the position along wi (tmin 0.001, tmax 100000).  A miss: sampled += T miss colour(wi).
 *      A hit on an emitting instance: sampled += T e' where dot(-normalize(wi), normal') > 0 (else + 0).  Nothing else of iteration 1 is done.
 * Per pixel, in frame order, every sum is a plain fp32 add per component (a sample adds + 0 to a sum it has nothing for); hits + 1 per sample
 * whose primary ray hit.  direct = seen + distant + sampled, in that order; the mean is direct / n. */
#define RENE_DIRECT_MAX_FRAMES 65536u
#define RENE_DIRECT_MISS 0u        /* rene_direct_sample.state: the primary ray hit nothing */
#define RENE_DIRECT_LIGHT 1u       /* the mixture took the light branch */
#define RENE_DIRECT_BSDF 2u        /* the mixture took the BSDF branch */
#define RENE_DIRECT_PLAIN 3u       /* no mixture: no emitter in the scene, or no diffuse lobe in the BSDF */
#define RENE_DIRECT_ENDED_PDF 4u   /* the sample ended at step 5 (pdf < 1e-5) */
#define RENE_DIRECT_ENDED_ZERO 5u  /* the sample ended at step 6 (T == 0) */
#define RENE_DIRECT_SECOND_NONE 0u     /* rene_direct_sample.second: no second query (a miss or an ended sample) */
#define RENE_DIRECT_SECOND_MISS 1u     /* the second ray left the scene */
#define RENE_DIRECT_SECOND_SURFACE 2u  /* ... hit an instance that does not emit */
#define RENE_DIRECT_SECOND_EMITTER 3u  /* ... hit an instance that emits (whichever side it was hit from) */
typedef struct rene_direct_params {
  uint32_t struct_size;  /* sizeof(rene_direct_params) */
  uint32_t first_frame;
  uint32_t n_frames;     /* 1 .. RENE_DIRECT_MAX_FRAMES */
  uint32_t flags;        /* reserved: 0 */
} rene_direct_params;
typedef struct rene_direct_pixel {  /* 48 bytes; the array is pixel-major [H][W], rows top first */
  float seen[3];         /* the sum of what the primary ray saw: the first hit's emission, or the miss colour */
  uint32_t hits;         /* samples whose primary ray hit */
  float distant[3];      /* the sum over the distant lights */
  uint32_t n;            /* n_frames for every pixel of a tile the context owns, 0 elsewhere (the all-zero record) */
  float sampled[3];      /* the sum of what the mixture ray found: T times the emission or the miss colour */
  uint32_t reserved;     /* 0 */
} rene_direct_pixel;
typedef struct rene_direct_sample {  /* 64 bytes: one sample of the pass */
  float seen[3];
  uint32_t state;        /* RENE_DIRECT_MISS .. _ENDED_ZERO */
  float distant[3];
  float pdf;             /* the mixed pdf, or s.pdf (0 for a miss) */
  float wi[3];           /* the mixture ray's direction (0 for a miss) */
  uint32_t second;       /* RENE_DIRECT_SECOND_* */
  float sampled[3];
  uint32_t reserved;     /* 0 */
} rene_direct_sample;
/* frames 0 .. 15 */
void rene_direct_params_default(rene_direct_params* out);
/* width x height x sizeof(rene_direct_pixel); host only */
size_t rene_direct_bytes(uint32_t width, uint32_t height);
/* The pass, into device_dst (device memory of the context's device, 16-byte aligned, at least rene_direct_bytes; all of those bytes are written:
 * zeroed, then the owned pixels' records) or, with device_dst == NULL, into a buffer the library owns (allocated by the first such call, outside
 * rene_plan_memory's figures, like the geometry pass's).  params == NULL: the defaults.
 * RENE_ERR_INVALID_ARGUMENT, before anything is launched: a NULL context, a struct_size that is not this build's, n_frames outside 1 .. 65536,
 * flags other than 0, a destination that is too small, misaligned or not device memory of the context's device.  RENE_ERR_UNSUPPORTED: the
 * context's scene selects the volpath integrator. */
int rene_direct(rene_ctx* ctx, const rene_direct_params* params, void* device_dst, size_t dst_bytes);
/* The library-owned result of the last rene_direct with device_dst == NULL (valid until the next such call or rene_destroy), and its download. */
int rene_direct_buffer(rene_ctx* ctx, void** device_ptr, size_t* n_bytes);
int rene_download_direct(rene_ctx* ctx, void* dst, size_t dst_bytes);
/* Probe: every sample the pass aggregates -- the same device functions -- as [n_frames][H][W] records in host memory (n = n_frames x width x
 * height records, at most 2^22).  The records of pixels in tiles the context does not own are all zero.  params as above. */
int rene_direct_samples(rene_ctx* ctx, const rene_direct_params* params, rene_direct_sample* host_dst, size_t n);

/* ---- the bounce pass: a job's radiance split by path depth, per pixel (build-defined; ABI v7, added symbols) --------------------------------------
 * How much of a pixel's radiance arrived at which iteration of the path loop, how long its paths were, and -- an option rene does not have -- the
 * same under a cap on the iterations.  The pass replays the WHOLE path estimator (lib.rs:141-357) from the seeds of frames first_frame ..
 * first_frame + n_frames - 1, one lane per pixel, in render_kernel's unfused form: a second statement of the estimator beside the render
 * kernels, which draws the random numbers the job's frames draw.  Path-integrator scenes only: a context whose scene selects volpath returns
 * RENE_ERR_UNSUPPORTED.  Opt-in: no other call's output changes.  Like the direct-light pass it reads nothing of the accumulation state and
 * changes nothing of it, runs on the context's stream, on tile shards and on adaptive contexts (the mask of active tiles plays no part);
 * rene_reset does not invalidate the result.
 *
 * The sample of pixel (px, py) under frame seed s, with cap D (max_depth; 0 means 50, rene's own):
 *   1. rng = PCG32si::new((py W + px) ^ s), whose first two f32 draws are the jitter; fw = PCG32si::new(s).  color = 1, i = 0, (ro, rd) the
 *      primary ray; ten values v[0 .. 9] = 0 (fp32 RGB).
 *   2. While i < D:
 *      a. The bucket b = min(i, 9); reached[b] += 1; length += 1.
 *      b. ONE closest-hit query of the main structure along (ro, rd) (tmin 0.001, tmax 100000).
 *      c. A miss: v[b] += color miss colour(rd) (the background colour times its texture; 0 without a background).  The sample ends (MISS).
 *      d. A hit: the closest-hit shader's surface; wo = -normalize(rd), normal = normalize(sf.normal); the BSDF as the render kernels build it.
 *         If the instance emits: v[b] += color e, where e is the emission if dot(wo, normal) > 0, else 0.
 *         For every distant light, in table order: wi = normalize((position + dir) - position); ONE any-hit query of the main structure from the
 *         position along wi (tmin 0.001, tmax 1e5); unoccluded: v[b] += ((color f(wo, wi)) |dot(wi, normal)|) L.
 *      e. The mixture (lib.rs:274-337).  With emit_object_len > 0 and a diffuse lobe in the BSDF: the coin from fw; > 0.5: the object
 *         fw.next_u32() % emit_object_len, the point from the emitter's sampler on fw, wi towards it, pdf = bsdf_pdf(wi, normal) (quirk Q1),
 *         f = f(wo, wi); else the BSDF's sample on rng.  Then the closest-hit query of the EMITTER structure along wi for pdf_l,
 *         color = color (f |dot(normal, wi)|), pdf = 0.5 pdf + 0.5 pdf_l / emit_object_len; pdf < 1e-5: the sample ends (PDF), else
 *         color = color / pdf.  Without emitters or without a diffuse lobe: the BSDF's sample s on rng; s.pdf < 1e-5: the sample ends (PDF),
 *         else color = color (s.f (|dot(normal, s.wi)| / s.pdf)).  (ro, rd) = (position, wi).
 *      f. color == 0 in all three components: the sample ends (ZERO; lib.rs:340-342).
 *      g. If i > 12: the roulette coin from fw; coin > max_element(color): the sample ends (ROULETTE), else color = color / max_element(color).
 *      h. i += 1.  If i >= D: the sample ends (CAP).
 * Per pixel, in frame order: bucket[d].sum += v[d], a plain fp32 add per component (a sample adds + 0 where it has nothing); reached,
 * length_sum (the closest-hit queries of the main structure) and capped (samples ended by CAP) are integer sums, length_max the maximum.
 * The radiance of the frames under the cap is ((b0 + b1) + b2) + ... over the ten sums; the first k of them are the radiance under a cap of k
 * (k <= 9), whatever D >= k the pass ran with. */
#define RENE_BOUNCES_MAX_FRAMES 65536u
#define RENE_BOUNCES_BUCKETS 10u
#define RENE_BOUNCES_MAX_DEPTH 50u     /* lib.rs:192 (Q7): the cap max_depth = 0 stands for, and the largest one */
#define RENE_BOUNCES_END_MISS 0u       /* rene_bounces_sample.end: the path left the scene */
#define RENE_BOUNCES_END_PDF 1u        /* ... ended at step e (pdf < 1e-5) */
#define RENE_BOUNCES_END_ZERO 2u       /* ... at step f (color == 0) */
#define RENE_BOUNCES_END_ROULETTE 3u   /* ... at step g */
#define RENE_BOUNCES_END_CAP 4u        /* ... at step h */
typedef struct rene_bounces_params {
  uint32_t struct_size;  /* sizeof(rene_bounces_params) */
  uint32_t first_frame;
  uint32_t n_frames;     /* 1 .. RENE_BOUNCES_MAX_FRAMES */
  uint32_t max_depth;    /* the cap D on a path's iterations: 1 .. 50, or 0 for 50 */
  uint32_t flags;        /* reserved: 0 */
} rene_bounces_params;
typedef struct rene_bounces_bucket {
  float sum[3];          /* d = 0 .. 8: what iteration d added; 9: what every iteration >= 9 added */
  uint32_t reached;      /* iterations counted into the bucket */
} rene_bounces_bucket;
typedef struct rene_bounces_pixel {  /* 176 bytes; the array is pixel-major [H][W], rows top first */
  rene_bounces_bucket bucket[RENE_BOUNCES_BUCKETS];
  uint32_t n;            /* n_frames for every pixel of a tile the context owns, 0 elsewhere (the all-zero record) */
  uint32_t length_sum;   /* iterations made, over all samples */
  uint32_t length_max;   /* the longest sample's */
  uint32_t capped;       /* samples ended by the cap */
} rene_bounces_pixel;
typedef struct rene_bounces_sample {  /* 176 bytes: one sample of the pass */
  rene_bounces_bucket bucket[RENE_BOUNCES_BUCKETS];  /* sum: v[d]; reached: the sample's own count */
  uint32_t n;            /* 1 (0 in the all-zero record of a pixel the context does not own) */
  uint32_t length;
  uint32_t end;          /* RENE_BOUNCES_END_* */
  uint32_t reserved;     /* 0 */
} rene_bounces_sample;
/* frames 0 .. 15, max_depth 0 */
void rene_bounces_params_default(rene_bounces_params* out);
/* width x height x sizeof(rene_bounces_pixel); host only */
size_t rene_bounces_bytes(uint32_t width, uint32_t height);
/* The pass, into device_dst (device memory of the context's device, 16-byte aligned, at least rene_bounces_bytes; all of those bytes are written:
 * zeroed, then the owned pixels' records) or, with device_dst == NULL, into a buffer the library owns (allocated by the first such call, outside
 * rene_plan_memory's figures, like the direct-light pass's).  params == NULL: the defaults.
 * RENE_ERR_INVALID_ARGUMENT, before anything is launched: a NULL context, a struct_size that is not this build's, n_frames outside 1 .. 65536,
 * max_depth above 50, flags other than 0, a destination that is too small, misaligned or not device memory of the context's device.
 * RENE_ERR_UNSUPPORTED: the context's scene selects the volpath integrator. */
int rene_bounces(rene_ctx* ctx, const rene_bounces_params* params, void* device_dst, size_t dst_bytes);
/* The library-owned result of the last rene_bounces with device_dst == NULL (valid until the next such call or rene_destroy), and its download. */
int rene_bounces_buffer(rene_ctx* ctx, void** device_ptr, size_t* n_bytes);
int rene_download_bounces(rene_ctx* ctx, void* dst, size_t dst_bytes);
/* Probe: every sample the pass aggregates -- the same device function -- as [n_frames][H][W] records in host memory (n = n_frames x width x
 * height records, at most 2^20).  The records of pixels in tiles the context does not own are all zero.  params as above. */
int rene_bounces_samples(rene_ctx* ctx, const rene_bounces_params* params, rene_bounces_sample* host_dst, size_t n);

/* ---- the light-group pass: a job's radiance split by the light it came from, per pixel (build-defined; ABI v7, added symbols) ----------------------
 * Which lamp, which distant light or the background put how much radiance into a pixel: what lets a finished job's lights be re-balanced without
 * rendering again.  The pass replays the bounce pass's sample (above, steps 1 and 2, with D = 50) from the seeds of frames first_frame ..
 * first_frame + n_frames - 1, one lane per pixel, and sends every add of the estimator to the GROUP of its source instead of a bucket:
 *   step c, the miss add                       -> group background_group
 *   step d, the hit instance's own emission    -> group instance_group[instance]   (an add is made wherever the instance carries an area light,
 *                                                 whatever its radiance: 0 where dot(wo, normal) <= 0)
 *   step d, distant light li                   -> group distant_group[li]
 * with up to RENE_LIGHTS_GROUPS groups; the tables are the caller's.  Each add's term (color e, ((color f) |dot|) L, color miss colour) is rounded
 * as a product of its own and then added.  A sample's value for a group is the fp32 fold of its adds to that group in the estimator's order,
 * starting from + 0; `adds` counts those with a non-zero component.  Per pixel, in frame order: group[g].sum += the sample's value, a plain fp32
 * add per component; adds is the integer sum; lit counts the samples with any non-zero add.  No sum is ever - 0, and a group nothing maps to, or
 * nothing reached, is all-zero words.  The radiance of the frames is ((g0 + g1) + g2) + ... over the eight sums -- the bounce pass's total in
 * another order of adding -- and a re-mix is the same fold with every group's sum times its weight.
 * Path-integrator scenes only (a volpath scene: RENE_ERR_UNSUPPORTED).  Opt-in, and on the bounce pass's terms otherwise: it reads and changes
 * nothing of the accumulation state, runs on the context's stream, on tile shards and on adaptive contexts; rene_reset does not invalidate the
 * result. */
#define RENE_LIGHTS_MAX_FRAMES 65536u
#define RENE_LIGHTS_GROUPS 8u
typedef struct rene_lights_params {
  uint32_t struct_size;  /* sizeof(rene_lights_params) */
  uint32_t first_frame;
  uint32_t n_frames;     /* 1 .. RENE_LIGHTS_MAX_FRAMES */
  uint32_t flags;        /* reserved: 0 */
  uint32_t n_instances;  /* entries of instance_group: the scene's instances */
  uint32_t n_distant;    /* entries of distant_group: the scene's distant lights */
  const uint8_t* instance_group;  /* host memory, every entry below RENE_LIGHTS_GROUPS (the entry of an instance without an area light is never read) */
  const uint8_t* distant_group;   /* host memory, likewise; may be NULL where n_distant is 0 */
  uint8_t background_group;       /* below RENE_LIGHTS_GROUPS */
} rene_lights_params;
typedef struct rene_lights_group {
  float sum[3];
  uint32_t adds;         /* adds to the group whose term had a non-zero component */
} rene_lights_group;
typedef struct rene_lights_pixel {  /* 144 bytes; the array is pixel-major [H][W], rows top first */
  rene_lights_group group[RENE_LIGHTS_GROUPS];
  uint32_t n;            /* n_frames for every pixel of a tile the context owns, 0 elsewhere (the all-zero record) */
  uint32_t lit;          /* samples with any non-zero add */
  uint32_t reserved[2];  /* 0 */
} rene_lights_pixel;
typedef struct rene_lights_sample {  /* 144 bytes: one sample of the pass */
  rene_lights_group group[RENE_LIGHTS_GROUPS];
  uint32_t n;            /* 1 (0 in the all-zero record of a pixel the context does not own) */
  uint32_t lit;          /* 0 | 1 */
  uint32_t length;       /* closest-hit queries of the main structure, as rene_bounces_sample.length */
  uint32_t end;          /* RENE_BOUNCES_END_* */
} rene_lights_sample;
/* frames 0 .. 15; both tables NULL with counts of 0 and background_group 0, which stands for the grouping of rene_lights_default_groups */
void rene_lights_params_default(rene_lights_params* out);
/* width x height x sizeof(rene_lights_pixel); host only */
size_t rene_lights_bytes(uint32_t width, uint32_t height);
/* The library's grouping of the context's scene, host only: group 0 is the background; then every distant light, in table order, a group each; then
 * every instance with an area light, in instance order, a group each; whatever does not fit below group 7 shares group 7.  Instances without an
 * area light get 0 (they never add).  instance_group has room for n_instances entries and distant_group for n_distant, which must be the
 * scene's counts (a table may be NULL where its count is 0); *n_used is the number of groups the grouping uses, 1 .. 8.  background_group and
 * n_used may be NULL. */
int rene_lights_default_groups(rene_ctx* ctx, uint8_t* instance_group, uint32_t n_instances, uint8_t* distant_group, uint32_t n_distant,
                               uint8_t* background_group, uint32_t* n_used);
/* The pass, into device_dst (device memory of the context's device, 16-byte aligned, at least rene_lights_bytes; all of those bytes are written:
 * zeroed, then the owned pixels' records) or, with device_dst == NULL, into a buffer the library owns (allocated by the first such call, outside
 * rene_plan_memory's figures, like the bounce pass's).  params == NULL: the defaults.  Params with both tables NULL and both counts 0 ask for
 * the grouping of rene_lights_default_groups (background_group is not read then).
 * RENE_ERR_INVALID_ARGUMENT, before anything is launched: a NULL context, a struct_size that is not this build's, n_frames outside 1 .. 65536,
 * flags other than 0, a count that is not the scene's, a NULL table with a count above 0, an entry of a table or a background_group of 8 or
 * more, a destination that is too small, misaligned or not device memory of the context's device.
 * RENE_ERR_UNSUPPORTED: the context's scene selects the volpath integrator. */
int rene_lights(rene_ctx* ctx, const rene_lights_params* params, void* device_dst, size_t dst_bytes);
/* The library-owned result of the last rene_lights with device_dst == NULL (valid until the next such call or rene_destroy), and its download. */
int rene_lights_buffer(rene_ctx* ctx, void** device_ptr, size_t* n_bytes);
int rene_download_lights(rene_ctx* ctx, void* dst, size_t dst_bytes);
/* Probe: every sample the pass aggregates -- the same device function -- as [n_frames][H][W] records in host memory (n = n_frames x width x
 * height records, at most 2^20).  The records of pixels in tiles the context does not own are all zero.  params as above. */
int rene_lights_samples(rene_ctx* ctx, const rene_lights_params* params, rene_lights_sample* host_dst, size_t n);

/* ---- multi-channel OpenEXR output: a job's layers in one file, packed on the device (build-defined; ABI v7, added symbols) ------------------------
 * The linear image, its guide layers, the denoised image and the geometry pass as ONE scan-line OpenEXR file, the format every compositor reads.
 * rene_output_exr turns what the context holds into the file's BODY -- the scan-line chunks in their final byte layout -- on the device, in a buffer
 * of the library's or in the caller's, so that only the file's bytes cross PCIe (6 to 66 per pixel, where the downloads of the same layers move
 * 128); rene_exr_header writes the header and the offset table, which follow from the film and the layer mask alone.  Opt-in: no other call's
 * output changes.
 *
 * The file: magic 20000630, version 2 (single part, scan lines); the attributes channels, compression (0: none), dataWindow and displayWindow
 * (0, 0, W - 1, H - 1), lineOrder (0: increasing y), pixelAspectRatio (1), screenWindowCenter (0, 0), screenWindowWidth (1), in that order, and a
 * terminating 0; an offset table of H little-endian uint64; then one chunk per scan line, rows top first: int32 y, int32 size = W * bytes_per_pixel,
 * and the row of every channel in turn, the channels ordered by the bytes of their names (capitals before `.`, digits and lower case), every channel
 * sampled 1 x 1.  Row y's chunk starts at y * (8 + W * bytes_per_pixel) of the body.  tests/test_images.py has an independent writer of the same
 * format, exr_bytes(channels, h, w, 0): header + body are its bytes.
 *
 * Layers (the mask `layers`), their channels and what a pixel holds:
 *   RENE_EXR_BEAUTY    R G B                      HALF   the mean of beauty_source -- RENE_OUTPUT_RADIANCE, _DENOISED_MEAN or _ROBUST -- as
 *                                                        rene_output_8bit defines the mean of that source: s / (float)N_t, N_t == 0 giving 0
 *   RENE_EXR_ALBEDO    albedo.R .G .B             HALF   rene_download_mean of layer 2
 *   RENE_EXR_NORMAL    normal.X .Y .Z             HALF   rene_download_mean of layer 1 (not renormalised)
 *   RENE_EXR_DENOISED  denoised.R .G .B           HALF   rene_download_denoised's RENE_DENOISED_MEAN of the last denoise call
 *   RENE_EXR_ALPHA     A                          HALF   (float)hits / (float)n of the geometry record (n == 0, a pixel no pass has filled: 0)
 *   RENE_EXR_DEPTH     Z                          FLOAT  depth_sum / (float)hits; hits == 0: +infinity
 *   RENE_EXR_POSITION  P.X .Y .Z                  FLOAT  position_sum / (float)hits; hits == 0: 0
 *   RENE_EXR_IDS       id0 .. id3, cov0 .. cov3   UINT, HALF   the record's id[k] and (float)count[k] / (float)n (n == 0: 0)
 * Every division is the correctly rounded fp32 one, denormals kept.  A HALF is the fp32 value clamped to +-65504 and then rounded to nearest, ties
 * to even, with fp16 subnormals kept (rene_export_features' rule for RENE_FEATURES_F16): no pixel is infinite, a NaN stays a NaN (the default quiet
 * NaN becomes 0x7e00), -0.0 keeps its sign.  The four geometry layers read the library-owned records of the context's last rene_gbuffer with
 * device_dst == NULL; rene_output_exr traces nothing itself.  rene_reset does NOT invalidate those records -- the pass reads the scene and the seed,
 * no frame of the context's -- so after a reset the geometry layers are still packed from them, beside layers of the new frames.
 *
 * rene_output_exr waits for the launches issued so far, runs on the context's stream and returns when the bytes are there; it writes nothing of the
 * accumulation state, of the denoiser's results or of the records.  Adaptive contexts: every pixel over its own tile's N_t.  On a RENE_SHARD_TILES
 * shard only the bytes of the owned tiles' pixels are written, and the 8-byte prefix of every row in which the shard owns a pixel; every other byte
 * of the destination is left as it was, so the tile shards of one device can fill one caller-owned buffer (every shard with records of its own
 * rene_gbuffer).  The destination is rene_output_8bit's: device_dst != NULL is a caller-owned device buffer of dst_bytes >= body_bytes, checked
 * before anything is launched (device memory of the context's device, 4-byte aligned, dst_bytes inside its allocation); device_dst == NULL is a
 * buffer of the library's own, zeroed on the context's stream when it is allocated, regrown or used with another mask, freed by rene_destroy and not
 * counted by rene_plan_memory (rene_exr_buffer, rene_download_exr; invalidated by rene_reset).  params == NULL: the defaults.
 * RENE_ERR_INVALID_ARGUMENT, nothing launched: a NULL context, a bad struct_size, a mask that is empty or has unknown bits, a beauty_source other
 * than the three above, a reserved word other than 0, a film outside 1 .. 16384 in either direction, a geometry layer without a library-owned
 * rene_gbuffer result of this context, DENOISED (or BEAUTY from _DENOISED_MEAN) and BEAUTY from _ROBUST before a valid result of their own calls
 * since the context was created or reset, a bad destination.
 * RENE_ERR_UNSUPPORTED: what rene_output_8bit refuses for the same sources -- a frame shard, a context whose chains an exchange has consumed until
 * its rene_reset, DENOISED and BEAUTY from _DENOISED_MEAN on a context with shard_count > 1. */
#define RENE_EXR_BEAUTY 1u
#define RENE_EXR_ALBEDO 2u
#define RENE_EXR_NORMAL 4u
#define RENE_EXR_DENOISED 8u
#define RENE_EXR_ALPHA 16u
#define RENE_EXR_DEPTH 32u
#define RENE_EXR_POSITION 64u
#define RENE_EXR_IDS 128u
#define RENE_EXR_ALL 255u
#define RENE_EXR_MAX_SIZE 16384u
typedef struct rene_exr_params {
  uint32_t struct_size;    /* sizeof(rene_exr_params) */
  uint32_t layers;         /* RENE_EXR_* mask */
  uint32_t beauty_source;  /* RENE_OUTPUT_RADIANCE, _DENOISED_MEAN or _ROBUST */
  uint32_t reserved;       /* 0 */
} rene_exr_params;
/* BEAUTY | ALBEDO | NORMAL, RADIANCE; host only */
void rene_exr_params_default(rene_exr_params* out);
/* The sizes of a width x height file of `layers`: the header with its offset table, the body (height x (8 + width x bytes_per_pixel)) and the bytes
 * a pixel takes in a chunk; any of the three pointers may be NULL.  Host only, no GPU needed.  RENE_ERR_INVALID_ARGUMENT: a bad mask or film. */
int rene_exr_layout(uint32_t width, uint32_t height, uint32_t layers, size_t* header_bytes, size_t* body_bytes, uint32_t* bytes_per_pixel);
/* The header and the offset table into host memory (dst_bytes >= header_bytes).  Host only, no GPU needed. */
int rene_exr_header(uint32_t width, uint32_t height, uint32_t layers, void* dst, size_t dst_bytes);
int rene_output_exr(rene_ctx* ctx, const rene_exr_params* params, void* device_dst, size_t dst_bytes);
/* The library-owned body of the last rene_output_exr with device_dst == NULL: its device pointer (valid until the next such call, rene_reset or
 * rene_destroy) and size in bytes, or a copy in host memory (dst_bytes >= that size).  RENE_ERR_INVALID_ARGUMENT before any such call since the
 * context was created or reset. */
int rene_exr_buffer(rene_ctx* ctx, void** device_ptr, size_t* n_bytes);
int rene_download_exr(rene_ctx* ctx, void* dst, size_t dst_bytes);
/* rene_output_exr into the library's buffer, then header, table and body into the file `path`.  RENE_ERR_IO: the file cannot be written. */
int rene_write_exr(rene_ctx* ctx, const rene_exr_params* params, const char* path);
/* The host form of the packing, the definition the device is held to: the body of a file of `layers` from planes of MEANS in host memory, rows top
 * first, tightly packed.  A plane whose layer is not in the mask is not read and may be NULL. */
typedef struct rene_exr_planes {
  uint32_t struct_size;    /* sizeof(rene_exr_planes) */
  uint32_t reserved;       /* 0 */
  const float* beauty;     /* [H][W][3] R G B */
  const float* albedo;     /* [H][W][3] */
  const float* normal;     /* [H][W][3] */
  const float* denoised;   /* [H][W][3] */
  const float* alpha;      /* [H][W] */
  const float* depth;      /* [H][W] */
  const float* position;   /* [H][W][3] */
  const uint32_t* ids;     /* [H][W][4] RENE_EXR_IDS: id0 .. id3 */
  const float* coverage;   /* [H][W][4] RENE_EXR_IDS: cov0 .. cov3 */
} rene_exr_planes;
/* RENE_ERR_INVALID_ARGUMENT: a bad mask, film or struct_size, a NULL plane of a chosen layer, a NULL dst, dst_bytes < body_bytes.  Host only. */
int rene_exr_body_host(uint32_t width, uint32_t height, uint32_t layers, const rene_exr_planes* planes, void* dst, size_t dst_bytes);

/* ---- compressed OpenEXR output: ZIPS chunks deflated on the device (build-defined; ABI v7, added symbols) ------------------------------------------
 * The same file with every scan line deflated before it crosses PCIe.  Opt-in through calls of its own: rene_output_exr, rene_exr_header,
 * rene_write_exr and rene_exr_params are what they were.  A compressed file is its ATTRIBUTES (rene_exr_attributes: the file from the magic through
 * the header's terminating 0, header_bytes - 8 x height bytes of rene_exr_layout) and its TAIL: the offset table of `height` little-endian uint64 --
 * absolute file offsets, the tail following the attributes -- and the chunks back to back, no padding.  The table depends on the data, so the
 * device writes it.  rene_exr_tail_bound = 8 x height + body_bytes is the tail's worst case; a call returns the bytes it wrote in *written, and the
 * file is attributes + tail[:written].
 *
 * The file: as the uncompressed one, except that the compression attribute's byte is 2 (ZIPS: one scan line per chunk).
 * Chunk y: int32 y, int32 size, then `size` bytes.  raw = the row's n = W x bytes_per_pixel bytes exactly as the uncompressed body holds them
 * behind its 8-byte prefix (n is even); z = the zlib stream below.  len(z) >= n: the chunk stores raw itself and size = n (the fallback every
 * reader detects by size == n); else it stores z.
 *   Pre-processing (OpenEXR's own):  t = raw[0::2] ++ raw[1::2];  d[0] = t[0], d[i] = (t[i] - t[i-1] + 128) mod 256.
 *   Tokens over d.  e[i] = (i >= 2 and d[i] == d[i-2]).  A position with e == 0 is a literal.  A maximal interval of e == 1 of length R is, from
 *   its start, R div 258 matches of length 258, then one match of length R mod 258 where that is >= 3, else R mod 258 literals.  Every match has
 *   distance 2.  (The greedy, non-lazy parse "longest match at distance 2, 3 .. 258 bytes", in a form that needs no sequential state: after the
 *   pre-processing a constant HALF channel is a run of one byte and a constant FLOAT or UINT channel a repeating byte pair.)
 *   Bits (RFC 1951).  One block, BFINAL = 1, BTYPE = 01: the first three bits, LSB first, are 1, 1, 0.  The fixed literal / length code: 0 - 143
 *   8 bits from 0x30, 144 - 255 9 bits from 0x190, 256 - 279 7 bits from 0, 280 - 287 8 bits from 0xC0; Huffman codes MSB first, extra bits LSB
 *   first; the standard length table (257 -> 3 ... 285 -> 258); the distance is always code 1, 5 bits, no extra bits; the end of the block is
 *   symbol 256, then zero bits to the byte boundary.
 *   zlib wrapper: the bytes 0x78 0x01, the block, Adler-32 of d big-endian.
 * Any inflate reads it.  ZIP (16-line chunks), dynamic Huffman codes and matches at other distances are not built.
 *
 * rene_exr_compress_host is the definition the device is held to: the tail of a width x height file of `layers` from an uncompressed body laid out
 * as rene_exr_body_host / rene_output_exr write it, in host memory; no GPU needed.  rene_exr_compress is the same on the context's device and
 * stream, from ANY device buffer that holds such a body -- width and height need not be the context's film -- which is what tile shards use: the
 * shards fill one caller-owned body with rene_output_exr, then one context compresses it.  It returns when the bytes are there.  device_dst:
 * device memory of the context's device, 8-byte aligned, dst_bytes >= rene_exr_tail_bound, not overlapping the body; its bytes beyond *written are
 * left as they were.  device_dst == NULL: a buffer of the library's own (rene_exr_tail_buffer, rene_download_exr_tail: tail[:written] and no more;
 * allocated by the first such call, freed by rene_destroy, invalidated by rene_reset, not counted by rene_plan_memory).
 * rene_output_exr_compressed is rene_output_exr into the library's body buffer (rene_exr_buffer hands it out afterwards as after that call), then
 * rene_exr_compress of it: rene_output_exr's refusals, and RENE_ERR_UNSUPPORTED on a context with shard_count > 1 -- a row spans tiles of several
 * shards; use rene_exr_compress.  rene_write_exr_compressed writes attributes + tail into `path`.
 * With RENE_EXR_COMPRESSION_NONE the calls produce the uncompressed file's bytes: the tail is rene_exr_header's table and the body.
 * RENE_ERR_INVALID_ARGUMENT, before anything is launched: a compression other than the two below, a bad mask or film, a NULL context, body, dst
 * (host form) or written, body_bytes other than rene_exr_layout's, dst_bytes below the bound, a body or destination that is misaligned, not device
 * memory of the context's device or shorter than its allocation says, a destination that overlaps the body (with device_dst == NULL: a body that
 * lies in the library's tail buffer). */
#define RENE_EXR_COMPRESSION_NONE 0u
#define RENE_EXR_COMPRESSION_ZIPS 2u   /* the file format's own codes */
/* 8 x height + body_bytes; 0 for a bad mask or film.  Host only. */
size_t rene_exr_tail_bound(uint32_t width, uint32_t height, uint32_t layers);
/* The attributes into host memory (dst_bytes >= header_bytes - 8 x height of rene_exr_layout).  Host only. */
int rene_exr_attributes(uint32_t width, uint32_t height, uint32_t layers, uint32_t compression, void* dst, size_t dst_bytes);
int rene_exr_compress_host(uint32_t width, uint32_t height, uint32_t layers, uint32_t compression, const void* body, size_t body_bytes, void* dst,
                           size_t dst_bytes, size_t* written);
int rene_exr_compress(rene_ctx* ctx, uint32_t width, uint32_t height, uint32_t layers, uint32_t compression, const void* device_body, size_t body_bytes,
                      void* device_dst, size_t dst_bytes, size_t* written);
int rene_exr_tail_buffer(rene_ctx* ctx, void** device_ptr, size_t* n_bytes);
int rene_download_exr_tail(rene_ctx* ctx, void* dst, size_t dst_bytes);
int rene_output_exr_compressed(rene_ctx* ctx, const rene_exr_params* params, uint32_t compression, void* device_dst, size_t dst_bytes, size_t* written);
int rene_write_exr_compressed(rene_ctx* ctx, const rene_exr_params* params, uint32_t compression, const char* path);
/* The same compression by row bytes, for a body that no layer mask describes (the Cryptomatte file below): `height` chunks of 8 + row_bytes bytes
 * in, the tail of a file whose attributes take attributes_bytes out -- the offset table holds absolute file offsets behind attributes_bytes, the
 * tail's worst case is 8 x height + body_bytes.  The kernels, the stream and the destination rules are rene_exr_compress's, and so are the
 * library-owned buffer and its accessors (rene_exr_tail_buffer, rene_download_exr_tail); with a mask's row bytes and attribute size the bytes are
 * rene_exr_compress's.  RENE_ERR_INVALID_ARGUMENT in addition: row_bytes that is 0, odd or above 16384 x 96, height outside 1 .. 16384,
 * body_bytes other than height x (8 + row_bytes). */
int rene_exr_compress_rows_host(uint32_t row_bytes, uint32_t height, size_t attributes_bytes, uint32_t compression, const void* body, size_t body_bytes,
                                void* dst, size_t dst_bytes, size_t* written);
int rene_exr_compress_rows(rene_ctx* ctx, uint32_t row_bytes, uint32_t height, size_t attributes_bytes, uint32_t compression, const void* device_body,
                           size_t body_bytes, void* device_dst, size_t dst_bytes, size_t* written);

/* ---- Cryptomatte output: id mattes by name, packed on the device (build-defined; ABI v7, added symbols) --------------------------------------------
 * The geometry pass's four id slots as a Cryptomatte file (specification 1.2.0), the id-matte format Nuke, Fusion, Blender and Natron read: ids are
 * hashes of NAMES stored as FLOAT, ranked by coverage, and a manifest in the header maps names to ids -- so two instances of one name are one
 * matte, and the file means something outside the process that built the scene.  A file and a set of calls of its own: rene_exr_layout /
 * rene_exr_header keep refusing mask bit 256, RENE_EXR_ALL stays 255, rene_gbuffer is what it was.
 *
 * Names.  rene_scene_instance_name / rene_scene_material_name hand out a loaded scene's; any list of n_names NUL-terminated UTF-8 strings over the
 * instance (or material) table will do -- a grouping per asset is just another list.  rene_scene_desc carries none: they are arguments here.
 *
 * The hash.  rene_cryptomatte_hash is MurmurHash3_x86_32 of the n bytes, seed 0, then with e = (h >> 23) & 255: e == 0 or e == 255 -> h ^= 1 << 23,
 * so that no id is a denormal, an infinity or a NaN.  The result is the FLOAT's bit pattern ("uint32_to_float32" is a reinterpretation).
 * hash("") = 00800000, hash("hello") = 248bfa47.  A layer's metadata KEY is the first 7 hex digits of %08x of its name's hash: CryptoObject
 * 3ae39a5, CryptoMaterial be359d6.
 * The manifest of a name list: {"<name>":"<%08x of its hash>",...} -- no spaces, names ordered by their bytes, each distinct name once, " and \
 * backslash-escaped, bytes below 0x20 as \u00XX, other bytes copied.  rene_cryptomatte_manifest writes it (no terminating 0) where dst_bytes
 * suffices and always stores its length in *written; dst == NULL asks for the length alone.
 *
 * The file is a scan-line OpenEXR as rene_exr_attributes writes one -- same magic, version 2, the same eight attributes in the same order -- with
 *   channels: per layer <L> two Cryptomatte levels of four FLOAT channels, <L>00.R = the id of rank 0, <L>00.G its coverage, <L>00.B the id of
 *     rank 1, <L>00.A its coverage; <L>01.* ranks 2 and 3 likewise: 32 bytes per pixel and layer.  The channel list and the rows of a chunk are
 *     in the order of the channel names' bytes (within a level A B G R, 00 before 01).  No preview channels <L>.R .G .B.
 *   attributes: behind screenWindowWidth, for every layer in the order of the layer names' bytes, four of type `string`:
 *     cryptomatte/<key>/conversion = uint32_to_float32, cryptomatte/<key>/hash = MurmurHash3_32, cryptomatte/<key>/manifest,
 *     cryptomatte/<key>/name = the layer's name.
 * 1 .. RENE_CRYPTOMATTE_MAX_LAYERS layers; a layer's name is 1 .. 24 bytes of [A-Za-z0-9_] that does not end in a digit, the names and their keys
 * distinct: every channel and attribute name fits 31 bytes.  id_source is RENE_GBUFFER_ID_INSTANCE or _MATERIAL (primitives have no names).
 * The file is attributes + the table of `height` uint64 + body (uncompressed), or attributes + rene_exr_compress_rows' tail with
 * row_bytes = width x bytes_per_pixel.  rene_cryptomatte_layout gives the sizes -- the manifest makes attributes_bytes depend on the names --
 * and rene_cryptomatte_attributes the bytes from the magic through the header's terminating 0.
 *
 * The body's values, per pixel and layer, from the layer's geometry record (count[k] of id[k], n):
 *   1. n == 0: eight zeros.
 *   2. slot k counts if count[k] > 0 and id[k] < n_names; its key is h_k = hash(names[id[k]]).  Any other slot is dropped.
 *   3. merge: k = 1, 2, 3 in turn, against j = 0 .. k - 1 in turn: where both count and h_k == h_j, count[j] += count[k] (uint32) and k is dropped.
 *   4. the counting slots are ordered by count descending, ties by key ascending as uint32.
 *   5. rank r holds the key's bits as the id and (float)count / (float)n as the coverage -- the correctly rounded fp32 division, denormals kept;
 *      an unused rank holds 0.0f, 0.0f.
 *   6. `other` and the misses are absent: a pixel's coverages add up to at most hits / n.
 * rene_cryptomatte_body_host is the definition the device is held to: host_records[l] is layer l's [H][W] record array in host memory.
 *
 * rene_output_cryptomatte packs the body on the device: a layer's `records` is a device pointer to its rene_gbuffer_pixel[H][W] (16-byte aligned,
 * memory of the context's device), or NULL for the library-owned result of the context's last rene_gbuffer with device_dst == NULL, whose
 * id_source must be the layer's.  n_names must be the context's instance (or material) count; an id out of range in a crafted record falls under
 * rule 2.  The pack traces nothing and writes nothing of the accumulation state or of the records; it waits for the launches issued so far, runs
 * on the context's stream and returns when the bytes are there.  The destination is rene_output_exr's: a caller-owned device buffer of dst_bytes
 * >= body_bytes, 4-byte aligned, of which a tile shard writes its own tiles' pixels and the 8-byte prefix of the rows it owns a tile in -- the
 * shards of one device fill one body -- or, with device_dst == NULL, a buffer of the library's own (rene_cryptomatte_buffer,
 * rene_download_cryptomatte; invalidated by rene_reset).  rene_write_cryptomatte packs into that buffer, compresses with rene_exr_compress_rows
 * and writes the file to path + ".tmp", then renames it to path; RENE_ERR_UNSUPPORTED on a context with shard_count > 1 as for
 * rene_output_exr_compressed, RENE_ERR_IO where the file cannot be written.
 * RENE_ERR_INVALID_ARGUMENT, before anything is launched: a NULL argument, a struct_size that is not this build's, n_layers outside 1 .. 3, a bad
 * layer name, equal names or keys, id_source _PRIMITIVE or unknown, a NULL name in a list, a film outside 1 .. RENE_EXR_MAX_SIZE, a destination too
 * small; on the device also: n_names that is not the context's count, records == NULL without a geometry result or with one of another id_source,
 * records or a destination that is misaligned or not device memory of the context's device. */
#define RENE_CRYPTOMATTE_MAX_LAYERS 3u
#define RENE_CRYPTOMATTE_MAX_NAME 24u
typedef struct rene_cryptomatte_layer {
  const char* name;          /* the layer's name, e.g. "CryptoObject" */
  uint32_t id_source;        /* RENE_GBUFFER_ID_INSTANCE or RENE_GBUFFER_ID_MATERIAL */
  uint32_t n_names;
  const char* const* names;  /* [n_names] names[i] is the name of id i */
  const void* records;       /* device: rene_gbuffer_pixel[H][W], or NULL: the library-owned result of the last rene_gbuffer (host calls ignore it) */
} rene_cryptomatte_layer;
typedef struct rene_cryptomatte_params {
  uint32_t struct_size;      /* sizeof(rene_cryptomatte_params) */
  uint32_t n_layers;         /* 1 .. RENE_CRYPTOMATTE_MAX_LAYERS */
  const rene_cryptomatte_layer* layers;
  uint64_t reserved;         /* 0 */
} rene_cryptomatte_params;
/* no layers: the caller fills n_layers and layers */
void rene_cryptomatte_params_default(rene_cryptomatte_params* out);
uint32_t rene_cryptomatte_hash(const char* utf8, size_t n);
int rene_cryptomatte_manifest(const char* const* names, uint32_t n_names, char* dst, size_t dst_bytes, size_t* written);
int rene_cryptomatte_layout(uint32_t width, uint32_t height, const rene_cryptomatte_layer* layers, uint32_t n_layers, size_t* attributes_bytes,
                            size_t* body_bytes, uint32_t* bytes_per_pixel);
int rene_cryptomatte_attributes(uint32_t width, uint32_t height, const rene_cryptomatte_layer* layers, uint32_t n_layers, uint32_t compression, void* dst,
                                size_t dst_bytes);
int rene_cryptomatte_body_host(uint32_t width, uint32_t height, const rene_cryptomatte_layer* layers, uint32_t n_layers,
                               const rene_gbuffer_pixel* const* host_records, void* dst, size_t dst_bytes);
int rene_output_cryptomatte(rene_ctx* ctx, const rene_cryptomatte_params* params, void* device_dst, size_t dst_bytes);
int rene_cryptomatte_buffer(rene_ctx* ctx, void** device_ptr, size_t* n_bytes);
int rene_download_cryptomatte(rene_ctx* ctx, void* dst, size_t dst_bytes);
int rene_write_cryptomatte(rene_ctx* ctx, const rene_cryptomatte_params* params, uint32_t compression, const char* path);

/* ---- OpenEXR pass layers: AO, direct, indirect, bounces, light groups, packed on the device (build-defined; ABI v7, added symbols) -----------------
 * What the occlusion, direct-light, bounce and light-group passes leave as 32- to 176-byte records, as the named HALF layers a compositor
 * re-balances: a file and a set of calls of its own, like the Cryptomatte file -- rene_exr_layout, rene_exr_header, rene_output_exr and
 * RENE_EXR_ALL stay what they are.  Only the file's bytes cross PCIe: 2 to 130 per pixel where the records take 400.
 *
 * The file is a scan-line OpenEXR as rene_exr_attributes writes one -- same magic, version 2, the same eight attributes in the same order, one chunk
 * per row (int32 y, int32 W x bytes_per_pixel, then every chosen channel's row), channels in the order of their names' bytes.  Every channel is
 * HALF, sampled 1 x 1.  The layers, in file order, and what a pixel of each holds -- every operation ONE fp32 operation: the IEEE division and
 * the correctly rounded square root, denormals kept, nothing contracted; (float) converts a uint32:
 *   RENE_EXRP_AO        ao                               rays ? 1 - (float)occluded / (float)rays : 1
 *   RENE_EXRP_BENT      bent.X .Y .Z                     l = sqrt((x x + y y) + z z) of bent_sum; l > 0 ? bent_sum / l : 0 (a NaN length: 0)
 *   RENE_EXRP_BOUNCES   depth0.B .G .R .. depth9.B .G .R n ? bucket[d].sum / (float)n : 0
 *   RENE_EXRP_DIRECT    direct.B .G .R                   n ? ((seen + distant) + sampled) / (float)n : 0
 *   RENE_EXRP_INDIRECT  indirect.B .G .R                 n ? (beauty_sum - ((seen + distant) + sampled)) / (float)n : 0, n the direct record's and
 *                                                        beauty_sum the context's radiance layer as rene_download(ctx, 0, ...) hands it out
 *   RENE_EXRP_LIGHTS    light0.B .G .R .. light7.B .G .R n ? group[g].sum / (float)n : 0, for the groups g of `groups` only
 *   RENE_EXRP_LENGTH    pathlength                       n ? (float)length_sum / (float)n : 0
 * (B, G, R are components 2, 1, 0 of a sum; X, Y, Z components 0, 1, 2.)  A value becomes a HALF by rene_output_exr's rule: clamped to +-65504,
 * rounded to nearest even, fp16 subnormals kept, - 0 keeps its sign.  A NaN stays a NaN and is written as the one pattern 0x7e00: which NaN an
 * fp32 operation makes of two infinities differs between processors (the sign, for one), so its bits are not the file's to carry.
 * `groups` is an 8-bit mask of the light groups to write; 0 means all eight, and it must be 0 without RENE_EXRP_LIGHTS.  bytes_per_pixel is 2 ..
 * 130.  group_names is NULL or eight entries, each NULL or 1 .. 24 bytes of [A-Za-z0-9_ -]: where a chosen group has a name the attributes gain,
 * behind screenWindowWidth, one `string` attribute rene/lightGroups = {"light0":"<name>",...} over the chosen groups that have one, in group
 * order, no spaces (the Cryptomatte manifest's shape; nothing in a name needs its escapes).  The channel names never change.  Without a name the
 * attribute is absent.  The uncompressed file is attributes + `height` uint64 offsets + body; the compressed one attributes + the tail of
 * rene_exr_compress_rows with row_bytes = width x bytes_per_pixel.  rene_exr_passes_layout gives the sizes (the names make attributes_bytes
 * depend on them) and rene_exr_passes_attributes the bytes from the magic through the header's terminating 0; both are host only.
 *
 * rene_exr_passes_body_host is the definition the device is held to: the four sources are HOST pointers to [H][W] records (those of the chosen
 * layers must be there), beauty_sum is [H][W][3] floats, or NULL without RENE_EXRP_INDIRECT.
 *
 * rene_output_exr_passes packs the body on the device.  A source is a device pointer to the caller's [H][W] record array of that pass (16-byte
 * aligned, memory of the context's device), or NULL: the library-owned result of the context's last call of that pass with device_dst == NULL.
 * A source whose layers are not chosen is not read.  The destination is rene_output_exr's: a caller-owned device buffer of dst_bytes >=
 * body_bytes, 4-byte aligned, checked before anything is launched, of which a RENE_SHARD_TILES shard writes its own tiles' pixels and the 8-byte
 * prefix of the rows it owns a tile in -- the shards of one device fill one body -- or, with device_dst == NULL, a buffer of the library's own
 * (rene_exr_passes_buffer, rene_download_exr_passes; zeroed when allocated, regrown or used with another layout, freed by rene_destroy,
 * invalidated by rene_reset, outside rene_plan_memory's figures).  The call waits for the launches issued so far, runs on the context's stream
 * and returns when the bytes are there.  It traces nothing and writes nothing of the accumulation state, the records or the denoiser's buffers.
 * rene_write_exr_passes packs into the library's buffer, compresses with rene_exr_compress_rows and writes the file to path + ".tmp", then renames
 * it to path; RENE_ERR_UNSUPPORTED on a context with shard_count > 1 as for rene_write_cryptomatte; a row beyond rene_exr_compress_rows' 16384 x 96
 * bytes is that call's refusal; RENE_ERR_IO where the file cannot be written.
 *
 * RENE_EXRP_INDIRECT's contract is that of beauty - direct: the radiance sums and the direct record must be sums over the SAME samples.  With
 * the library-owned direct result the library checks what it can -- the context's frame_base is that pass's first_frame, and every owned tile's
 * N_t is its n_frames; an adaptive context with uneven tiles is therefore refused.  A context whose renders were not one contiguous range but
 * happen to match the counts is not detected.  With a caller's `direct` source there is nothing to check N_t against: the contract is the
 * caller's.
 * RENE_ERR_INVALID_ARGUMENT, before anything is launched: a NULL context or params, a struct_size that is not this build's, an empty mask or
 * unknown bits, groups above 255 or set without RENE_EXRP_LIGHTS, a bad name, a non-zero reserved word, a film outside 1 .. RENE_EXR_MAX_SIZE, a
 * chosen layer whose source is NULL where the context has no library-owned result of that pass, a source or destination that is misaligned, too
 * small or not this device's memory, RENE_EXRP_INDIRECT when the context's frames are not the direct result's.  RENE_ERR_UNSUPPORTED, with
 * RENE_EXRP_INDIRECT: what rene_output_exr refuses for RENE_OUTPUT_RADIANCE -- a frame shard, or chains consumed by an exchange. */
#define RENE_EXRP_AO 1u
#define RENE_EXRP_BENT 2u
#define RENE_EXRP_BOUNCES 4u
#define RENE_EXRP_DIRECT 8u
#define RENE_EXRP_INDIRECT 16u
#define RENE_EXRP_LIGHTS 32u
#define RENE_EXRP_LENGTH 64u
#define RENE_EXRP_ALL 127u
#define RENE_EXRP_MAX_NAME 24u
typedef struct rene_exr_passes_params {
  uint32_t struct_size;            /* sizeof(rene_exr_passes_params) */
  uint32_t layers;                 /* RENE_EXRP_* mask, not empty */
  uint32_t groups;                 /* the light groups RENE_EXRP_LIGHTS writes, 8 bits; 0: all eight */
  uint32_t reserved;               /* 0 */
  const char* const* group_names;  /* NULL, or 8 entries: NULL or the group's name */
  const void* occlusion;           /* rene_occlusion_pixel[H][W], or NULL: the library-owned result (device; host for rene_exr_passes_body_host) */
  const void* direct;              /* rene_direct_pixel[H][W], likewise */
  const void* bounces;             /* rene_bounces_pixel[H][W], likewise */
  const void* lights;              /* rene_lights_pixel[H][W], likewise */
} rene_exr_passes_params;
/* all seven layers, groups 0, no names, no sources */
void rene_exr_passes_params_default(rene_exr_passes_params* out);
int rene_exr_passes_layout(uint32_t width, uint32_t height, const rene_exr_passes_params* params, size_t* attributes_bytes, size_t* body_bytes,
                           uint32_t* bytes_per_pixel);
int rene_exr_passes_attributes(uint32_t width, uint32_t height, const rene_exr_passes_params* params, uint32_t compression, void* dst, size_t dst_bytes);
int rene_exr_passes_body_host(uint32_t width, uint32_t height, const rene_exr_passes_params* params, const float* beauty_sum, void* dst, size_t dst_bytes);
int rene_output_exr_passes(rene_ctx* ctx, const rene_exr_passes_params* params, void* device_dst, size_t dst_bytes);
int rene_exr_passes_buffer(rene_ctx* ctx, void** device_ptr, size_t* n_bytes);
int rene_download_exr_passes(rene_ctx* ctx, void* dst, size_t dst_bytes);
int rene_write_exr_passes(rene_ctx* ctx, const rene_exr_passes_params* params, uint32_t compression, const char* path);

int rene_get_stats(rene_ctx* ctx, rene_stats* out);

/* Batch closest-hit queries against the main (which == 0) or emitter-only (which == 1) structure;
 * host pointers; 0 <= tmin <= tmax.  Exposes the traversal the Vulkan driver hides. */
int rene_trace(rene_ctx* ctx, int which, size_t n, const float* origins, const float* directions,
               float tmin, float tmax, rene_hit* out);

/* The J1 gate (probes, no reference counterpart): what does traversal alone cost when its rays come from a queue?
 * rene_ray_dump renders frames [first_frame, first_frame + n_frames) on a RENE_FLAG_COUNTERS context of a deep-BVH path-integrator scene and
 * records every traversal query the launch issues -- 8 floats per ray: o.xyz, tmax, d.xyz, bits(pixel | depth << 21 | any-hit << 27 | emitter
 * structure << 28 | (frame & 7) << 29) -- up to `capacity` rays into host memory; *n_issued = the queries issued (may exceed capacity).  The frames are accumulated
 * like any rendered frames.  rene_trace_queue runs a traversal-only persistent pass over n rays in queue order (origin + tmax as 4 floats; the
 * direction as three halves + flags in the fourth half (fp16 != 0, 8 bytes per ray) or three floats + flags (16 bytes); flag bit 0 any-hit,
 * bit 1 emitter-only structure): free lanes are refilled from the queue as soon as `refill_min` of a wave's 64 are free; `repeats` timed
 * launches, *ms = the fastest; hits4 (optional): t (-1 = miss), u, v, bits(slot) per ray; steps5 (optional): wave-steps and lane-steps of the
 * node and leaf steps + iterations. */
int rene_ray_dump(rene_ctx* ctx, uint32_t first_frame, uint32_t n_frames, size_t capacity, float* rays8, uint64_t* n_issued);
int rene_trace_queue(rene_ctx* ctx, size_t n, const float* o_tmax4, const void* d_flags, int fp16, uint32_t refill_min, uint32_t leaf_min,
                     uint32_t blocks_per_cu, uint32_t repeats, float* hits4, float* ms, uint64_t* steps5);

/* Per-function probe of the device BSDF code (EnumMaterial::compute_bsdf + Bsdf::{f, pdf, sample_f},
 * rene-shader/src/material.rs:739-769, reflection.rs:286-342): for each of the n items builds the
 * lobes of `material_index` at (normal, uv) and writes 12 floats: f(wo,wi).rgb, pdf(wo,wi),
 * sample.wi.xyz, sample.f.rgb, sample.pdf (one sample_f(wo) from PCG32si::new(seed)), lobe count.
 * Host pointers; world-space directions. */
int rene_bsdf_eval(rene_ctx* ctx, uint32_t material_index, size_t n, const float* normals3,
                   const float* uvs2, const float* wo3, const float* wi3, const uint32_t* seeds,
                   float* out12);

/* Per-function probe of the device medium code (EnumMedium::{tr, phase, sample, sample_p},
 * rene-shader/src/medium.rs:104-158) for n items with ray origin 0.  Writes 16 floats per item:
 * tr(rd, t_max).rgb, phase(wo, wi), sample.sampled (0/1), sample.position.xyz, sample.tr.rgb,
 * sample_p(wo).xyz (drawn after `sample` from the same PCG32si::new(seed)), the bits of the stream's
 * next u32, 0.  Host pointers.  RENE_ERR_INVALID_ARGUMENT unless the scene's integrator is volpath. */
int rene_medium_eval(rene_ctx* ctx, uint32_t medium_index, size_t n, const float* rd3,
                     const float* t_max, const float* wo3, const float* wi3, const uint32_t* seeds,
                     float* out16);

/* Probe of the transmittance walks (tr / tr_emit, rene-shader/src/lib.rs:359-468) for n rays that start in
 * medium `medium_index`: the walk through None-material boundaries, each crossing switching the medium by
 * dot(direction, normal) > 0 and restarting at the hit position with tmin 0.001; emit != 0 is tr_emit (a miss is 0,
 * the first area light returns its radiance where it faces the ray).  Runs on the item loop or the BVH as the context's
 * scene and flags select, like rene_trace.  Writes 4 floats per ray: tr.rgb and the number of closest-hit queries the
 * walk traced.  Host pointers.  RENE_ERR_INVALID_ARGUMENT unless the scene's integrator is volpath, or for an index
 * past the media.  Added without an ABI version change. */
int rene_transmittance(rene_ctx* ctx, int emit, uint32_t medium_index, size_t n, const float* origins,
                       const float* directions, float* out4);

/* Per-function probe of the emitter-pdf query (rene-shader/src/lib.rs:301-318: trace `direction` from `origin`
 * against the emitter-only structure, tmin 0.001, tmax 1e5, then main_miss_pdf / triangle_closest_hit_pdf /
 * sphere_closest_hit_pdf, lib.rs:959-1066): out[i] = pdf_l of ray i (0 on a miss).  Host pointers. */
int rene_emitter_pdf(rene_ctx* ctx, size_t n, const float* origins, const float* directions, float* out);

/* The same query in the form a render kernel runs it.  form 0: rene_emitter_pdf (the global tables, item loop or BVH as the context's
 * scene and flags select).  form 1: what the small-scene render kernels run -- the item loop over the emitter items with the winning
 * item looked up in the LDS image, then the pdf from the image's per-slot emitter records.  form 2: form 1 with the direction normalised
 * first and handed on as it is (the kernels that share normalize(rd) between the pdf and the hit branch).  Forms 1 and 2 return
 * RENE_ERR_INVALID_ARGUMENT unless the context's kernels are small-scene ones (rene_scene_pack_info: FEAT_SMALL, and no RENE_FLAG_FORCE_BVH).
 * Added without an ABI version change. */
int rene_emitter_pdf_form(rene_ctx* ctx, int form, size_t n, const float* origins, const float* directions, float* out);

/* Per-function probe of emitter sampling (EnumSurfaceSample::sample, rene-shader/src/surface_sample.rs:69-117, behind the object choice of
 * lib.rs:279-283): for each of the n seeds, fw = PCG32si::new(seed), obj = fw.next_u32() % emit_object_len, the point on that object.
 * Writes 8 floats per item: the point's xyz, the bits of obj, the bits of the stream's next u32, 0, 0, 0.  form 0 reads the global tables,
 * form 1 the LDS image of a small scene (RENE_ERR_INVALID_ARGUMENT unless the context's kernels are small-scene ones).  Both forms return
 * RENE_ERR_INVALID_ARGUMENT for a scene without emitters.  Host pointers.  Added without an ABI version change. */
int rene_emit_sample(rene_ctx* ctx, int form, size_t n, const uint32_t* seeds, float* out8);

/* Probe of the device random stream (PCG32si, rene-shader/src/rand.rs:4-52): out[k] = the k-th next_u32() of
 * PCG32si::new(seed) computed by one lane of `device`.  Integer-exact known answers: tests/golden/pcg32si_kat.json. */
int rene_pcg_probe(int device, uint32_t seed, uint32_t n, uint32_t* out);

/* Probe of the frame-stream table.  The kernels of small Matte-only scenes (triangle emitters, no textures, no background) do not draw the
 * reference's frame-wide sample stream (PCG32si::new(frame seed): the light / BSDF coin, the emitter point, the roulette number of
 * lib.rs:274-324, 345-354) in every lane: a small kernel walks it once per launch frame and the render kernel reads the result.  This call
 * runs that kernel for global frames first_frame .. first_frame + n_frames - 1 of the context's seed and scene and downloads what it wrote:
 * out[n_frames][50][4] floats, depth-major per frame --
 *   x, y, z  the sampled point on an emitter (0 where the coin says BSDF or the scene has no emitter, in which case no coin is drawn)
 *   w        the roulette number of that depth (0 up to depth 12: none is drawn), its sign bit set where the coin says light (pcg_f32 > 0.5).
 * Host pointer.  RENE_ERR_INVALID_ARGUMENT for a scene whose kernel draws the stream per lane, or more than 65536 frames. */
int rene_frame_stream_probe(rene_ctx* ctx, uint32_t first_frame, uint32_t n_frames, float* out);

/* Probe of the passes over the frame chains: puts the CALLER'S chains into a context, so that a test can hand the resolve, rene_download_mean,
 * rene_estimate_noise, rene_resolve_robust, rene_export_features and rene_denoise sums no render would leave -- ties, NaN, infinities, denormals,
 * -0.0 -- on any tile grid.  chains: a host pointer to [8][3][yres][xres][3] floats (n_floats of them at least) -- chain, then layer (RENE_LAYER_*),
 * rows top first, tightly packed RGB.  The pixels of the tiles the context OWNS are scattered into its chain memory on the host and copied on the
 * context's stream (no kernel), bit for bit: NaN payloads, -0.0 and denormals arrive as they are.  The slots of ragged tiles outside the image stay
 * zero, and the fourth float of every record, the library's version word, is what rene_reset leaves there.
 * The bookkeeping is what rene_render(first_frame, n_frames) leaves on a freshly reset context: rene_stats.frames, the chains' frame counts (frame
 * f in chain f mod 8: the data of a chain the range leaves empty should be zero, as a render leaves it), the first frame, and the next hand-out
 * resolves the loaded chains; nothing was rendered, so rene_stats.paths, .launches and the ray counters stay 0.  tile_frames == NULL: every tile
 * holds the n_frames frames.  Otherwise n_tiles == tiles_y * tiles_x and tile t of the full grid, row-major, holds the frames [first_frame,
 * first_frame + tile_frames[t]), each <= n_frames and at least one equal to it: the state an adaptive job leaves (rene_set_active_tiles), tiles
 * with N_t == 0 included; a tile shard looks at the entries of its own tiles (its rene_stats.frames is the largest of them).
 * Afterwards every call that reads the accumulation state works as after a render (rene_download, rene_download_mean, rene_framebuffer,
 * rene_tile_frames, rene_estimate_noise, rene_resolve_robust, rene_export_features, rene_denoise and its three variants, each with its own refusals);
 * rene_render and
 * rene_set_active_tiles return RENE_ERR_UNSUPPORTED until rene_reset: the version words no longer describe the sums.
 * RENE_ERR_INVALID_ARGUMENT: a NULL ctx or chains, n_floats too small, n_frames == 0 (or a frame range beyond 2^32 - 1), a bad tile_frames (n_tiles,
 * an entry above n_frames, none equal to it), a context that already holds frames (rene_reset first).  RENE_ERR_UNSUPPORTED: a frame shard
 * (RENE_SHARD_FRAMES with shard_count > 1), and a context whose chains an exchange has consumed until its rene_reset.  Nothing is written on a refusal. */
int rene_load_chains(rene_ctx* ctx, const float* chains, size_t n_floats, uint32_t first_frame, uint32_t n_frames,
                     const uint32_t* tile_frames, size_t n_tiles);

/* ---- checkpoint of a render job: save, restore and resume it bit for bit (build-defined; ABI v7, added symbols) ----------------------------------
 * A job's whole worth is the eight frame chains of its context.  These calls take them out and put them back so that rendering GOES ON: the chain
 * rule is a rule on the frame's number, the seeds follow from the frame number, and a context after rene_reset carries version 0 on every record --
 * so a fresh context whose chains hold the saved sums continues exactly as the original would have.  The interrupted job is bit for bit the
 * uninterrupted one, in every layer, on every kernel family and under adaptive sampling.  A state is written tile by tile, so it restores on any
 * tile-shard layout: one part into several shards, several shards' parts into one context.
 *
 * The state format, version 1.  Little-endian; every reserved byte is zero.  A PART is what one context saves:
 *   rene_state_header                      256 bytes
 *   rene_state_tile [n_tiles]              32 bytes per tile of the part, in strictly ascending order of `tile`
 *   payload, per tile in table order       RENE_STATE_TILE_BYTES = 294912 bytes: float [8 chains][3 layers][32 dy][32 dx][3], the layers in RENE_LAYER_*
 *                                          order, the pixels ROW-MAJOR inside the tile (not in the device's slot order), pixels outside the image
 *                                          zero.  The records' version words are not stored.  The bits travel as they are: NaN payloads, -0.0,
 *                                          denormals.
 * The checksum of a tile, over its 73728 payload dwords w_i (uint32, i = 0 .. 73727 in payload order): c0 = sum of w_i, c1 = sum of (i + 1) w_i,
 * both mod 2^32 -- integer sums, the same in any reduction order.
 * The scene fingerprint (rene_scene_fingerprint): 128 bits over the tables of the rene_scene_desc as rene_create receives them, independent of how
 * the library packs them, so that a later build accepts the file.  The desc is read as a stream of uint32 words s_0, s_1, ...:
 *   integrator, xresolution, yresolution, the 53 words of the uniform, n_instances, n_meshes, n_materials, n_textures, n_area_lights, n_lights,
 *   n_images, n_mediums; the instances (18 words each); per mesh n_vertices, n_indices, its vertices (8 words each), its indices; the materials
 *   (13 words each), textures (9), area lights (5), lights (9); per image width, height, its 4 width height floats; the mediums (9 words each)
 * -- floats as their bit patterns.  With a = 0x243F6A8885A308D3, b = 0x13198A2E03707344 (uint64, arithmetic mod 2^64) every word does
 *   a = (a ^ s) * 0x00000100000001B3;   b = (rotl(b, 27) + s) * 0x9E3779B97F4A7C15
 * and at the end a and b each go through h ^= h >> 33; h *= 0xFF51AFD7ED558CCD; h ^= h >> 33.  out[0] = a, out[1] = b.  Every step is a bijection
 * of the state, so two descs that differ in one word differ in their fingerprints.
 *
 * What is and is not restored.  Restored: the chains' sums, the first frame F, every tile's frame count N_t and whether it is active, the chains'
 * frame counts, rene_stats.frames and .paths, and whether the chains came from rene_load_chains.  NOT restored: rene_stats.launches, the ray
 * counters and the timings, which count what THIS context itself does; results of the passes (the denoiser's, the noise estimate's ...), which
 * their calls compute again; rene_tune's choice. */
#define RENE_STATE_MAGIC 0x54534E52u /* "RNST" */
#define RENE_STATE_VERSION 1u
#define RENE_STATE_TILE_BYTES 294912u /* 8 chains, 3 layers, 32 x 32 pixels, 12 bytes */
#define RENE_STATE_TILE_ACTIVE 1u     /* rene_state_tile.flags, bit 0: the tile was rendering when the state was saved */
typedef struct rene_state_header {
  uint32_t magic;              /* RENE_STATE_MAGIC */
  uint32_t version;            /* RENE_STATE_VERSION */
  uint32_t header_bytes;       /* 256 */
  uint32_t tile_size;          /* RENE_TILE_SIZE */
  uint32_t width, height;      /* the film */
  uint32_t tiles_x, tiles_y;   /* ceil(width / 32), ceil(height / 32) */
  uint32_t seed;               /* rene_opts.seed */
  uint32_t frame_base;         /* F: the first frame rendered */
  uint32_t n_frames;           /* N: the largest N_t in the part (of a context that owns no tile: its rene_stats.frames); chain_frames are the
                                  counts of the frames [F, F + N) */
  uint32_t frames_contiguous;  /* 1: the frames so far are the one range [F, F + N) */
  uint32_t loaded;             /* 1: the chains came from rene_load_chains; nothing renders onto them */
  uint32_t n_tiles;            /* tiles in this part */
  uint64_t paths;              /* rene_stats.paths */
  uint64_t chain_frames[8];    /* the frames every chain has received */
  uint64_t fingerprint[2];     /* rene_scene_fingerprint of the scene */
  uint64_t payload_offset;     /* header_bytes + 32 n_tiles */
  uint64_t total_bytes;        /* payload_offset + RENE_STATE_TILE_BYTES n_tiles */
  uint8_t reserved[96];
} rene_state_header;
typedef struct rene_state_tile {
  uint32_t tile;               /* ty * tiles_x + tx on the image's full tile grid */
  uint32_t n_frames;           /* N_t: the tile holds the frames [F, F + N_t) */
  uint32_t flags;              /* RENE_STATE_TILE_ACTIVE */
  uint32_t c0, c1;             /* the checksum of the tile's payload */
  uint32_t reserved[3];
} rene_state_tile;
/* what rene_state_inspect reads from a part's header */
typedef struct rene_state_info {
  uint32_t struct_size;        /* sizeof(rene_state_info) */
  uint32_t version;
  uint32_t width, height, tile_size, tiles_x, tiles_y;
  uint32_t seed, frame_base, n_frames, frames_contiguous, loaded, n_tiles;
  uint32_t reserved;
  uint64_t paths;
  uint64_t chain_frames[8];
  uint64_t fingerprint[2];
  uint64_t payload_offset, total_bytes;
} rene_state_info;
typedef struct rene_state_params {
  uint32_t struct_size;        /* sizeof(rene_state_params) */
  uint32_t chunk_tiles;        /* owned tiles per chunk of the device <-> host pipeline; 0: the default, 128 (37.7 MB).  Changes no byte of any result */
  uint32_t reserved[2];
} rene_state_params;
/* chunk_tiles 0; host only */
void rene_state_params_default(rene_state_params* out);
/* Host only: the fingerprint specified above.  RENE_ERR_INVALID_ARGUMENT: a NULL argument, a bad struct_size, a NULL table with a count above 0. */
int rene_scene_fingerprint(const rene_scene_desc* scene, uint64_t out[2]);
/* Host only: the bytes of the part a context of shard `shard_rank` of `shard_count` (tile shards; 0, 1: unsharded) saves for a width x height film;
 * 0 for an empty film, a resolution above 16384, shard_count == 0 or shard_rank >= shard_count. */
size_t rene_state_bytes(uint32_t width, uint32_t height, uint32_t shard_rank, uint32_t shard_count);
/* Saves the context's state into host memory: dst_bytes >= rene_state_bytes of the context, *written (may be NULL) = the part's bytes.  Waits for the
 * launches issued so far; reads the chains and writes nothing of the accumulation state.  The chains are packed on the device, chunk_tiles owned
 * tiles at a time, through two device chunk buffers and two pinned stagings, so that the kernel of one chunk runs under the copy of the one before:
 * memory the first call allocates, rene_destroy frees and rene_plan_memory does not count (two times chunk_tiles x 294912 bytes on either side, and
 * 8 bytes per owned tile).  Allowed on a context filled by rene_load_chains: the flag travels with the state.
 * RENE_ERR_UNSUPPORTED: a frame shard (RENE_SHARD_FRAMES with shard_count > 1); a context whose chains an exchange has consumed.
 * RENE_ERR_INVALID_ARGUMENT: a NULL argument, bad params, a context without frames, a destination that is too small, more than 2^32 - 1 frames. */
int rene_save_state(rene_ctx* ctx, const rene_state_params* params, void* dst, size_t dst_bytes, size_t* written);
/* Restores a state into a FRESH context (created or reset, no frames: what rene_load_chains demands) from one or more parts in host memory.
 * Everything is validated before anything is written:
 *   every part passes rene_state_inspect; its film, seed and fingerprint are the context's; F, frames_contiguous and loaded agree in all parts,
 *   and chain_frames in all parts of the largest N (the part of a tile shard whose tiles all stopped before the job's last frame has a smaller N
 *   and the counts of that N; its tiles are all inactive); every tile the context owns is present exactly once across the parts (tiles it does not own are ignored); with N the largest N_t in
 *   the given parts, every active tile has N_t == N; a state with stopped tiles does not go into a RENE_FLAG_WAVEFRONT context unless it is loaded.
 * Then the payloads are uploaded chunk by chunk and unpacked on the device into records that carry the version word rene_reset leaves; slots
 * outside the image are zero.  Afterwards the bookkeeping is what rene_load_chains leaves for first_frame F, n_frames N and the tiles' N_t, but:
 * the tiles' active flags come from the table; rene_stats.paths and the chains' frame counts come from the headers (the paths: their sum where
 * every given tile is owned, else the sum of N_t x the pixels of the owned tiles); `loaded` is the header's -- a state saved from a rendered
 * context RENDERS ON: the next frame is F + N -- and rene_set_active_tiles works under its usual rules (the set only shrinks).
 * rene_stats.launches, the ray counters and the timings count what this context itself does.
 * The device recomputes every tile's checksum from what arrived; a mismatch is therefore found only after the upload: the context is then left
 * as rene_reset leaves it and the error (RENE_ERR_INVALID_ARGUMENT) names the tile.
 * RENE_ERR_UNSUPPORTED: a frame shard; an exchanged context.  RENE_ERR_INVALID_ARGUMENT: everything else above; nothing is written then. */
int rene_restore_state(rene_ctx* ctx, const rene_state_params* params, const void* const* parts, const size_t* part_bytes, size_t n_parts);
/* Host only: fills *out from a part's header after checking the whole part's consistency -- magic, version, sizes, the tile grid, bytes ==
 * total_bytes (a truncated part is named as such), reserved bytes, and the tile table: ascending tile indices inside the grid (a duplicate and
 * tiles out of order are told apart), no N_t above N, one equal to it, every active tile at N.  RENE_ERR_INVALID_ARGUMENT with a message. */
int rene_state_inspect(const void* blob, size_t bytes, rene_state_info* out);
/* Host only: the part's tile table (n >= n_tiles entries at dst), after the checks of rene_state_inspect. */
int rene_state_tiles(const void* blob, size_t bytes, rene_state_tile* dst, size_t n);
/* Host only: rene_state_inspect, then every tile's checksum recomputed from its payload; a mismatch names the tile. */
int rene_state_verify(const void* blob, size_t bytes);
/* Host only: rene_state_inspect and rene_state_tiles of a part in a FILE, of which only header and table are read (tiles may be NULL; else n >=
 * n_tiles entries): what a caller needs to know of a checkpoint before or after it restores it.  RENE_ERR_IO: a file that cannot be read. */
int rene_state_inspect_file(const char* path, rene_state_info* out, rene_state_tile* tiles, size_t n);
/* The same two calls streamed chunk by chunk to and from files: host memory stays at the two stagings, whatever the film's size.  Saving writes
 * to `path` + ".tmp" and renames it onto `path` when it is complete: a file is whole or absent.  RENE_ERR_IO: a file that cannot be opened, read,
 * written or renamed. */
int rene_save_state_file(rene_ctx* ctx, const rene_state_params* params, const char* path);
int rene_restore_state_files(rene_ctx* ctx, const rene_state_params* params, const char* const* paths, size_t n_paths);

/* ---- multi-GPU exchange step inside the boundary: RCCL over xGMI ---------------------------------
 * The reference renders on one GPU; this build shards a job over the GPUs of a node (one context per GPU; tiles or
 * frame blocks, rene_opts.shard_*) and needs exactly one exchange at the end of a job -- the sum of the per-GPU
 * accumulation images (SURVEY section 8 e).  These entry points keep it on the device: ncclReduce / ncclSend /
 * ncclRecv on the context's own stream, ordered after its launches.  RCCL (librccl.so) is loaded when the first of
 * them is called; RENE_ERR_UNSUPPORTED if it is absent.
 *   one process per GPU:  rank 0 calls rene_comm_unique_id and hands the 128 bytes to the other ranks by whatever means
 *                         the host has (a file, a socket, torch.distributed's store); every rank then calls rene_comm_init;
 *   one process, n GPUs:  rene_comm_init_all over its n contexts (ncclCommInitAll); calls on different contexts of one
 *                         communicator must then be made from different host threads or inside rene_comm_group_begin /
 *                         rene_comm_group_end (ncclGroupStart / ncclGroupEnd).
 * After an exchange the root's image holds the job's sums; every context of the communicator needs rene_reset before
 * it renders again (the records' version words have been summed or overwritten). */
#define RENE_COMM_ID_BYTES 128
int rene_comm_unique_id(uint8_t id[RENE_COMM_ID_BYTES]);
int rene_comm_init(rene_ctx* ctx, int n_ranks, int rank, const uint8_t id[RENE_COMM_ID_BYTES]);
int rene_comm_init_all(rene_ctx** ctxs, int n);
int rene_comm_group_begin(void);
int rene_comm_group_end(void);
/* Frame-sharded jobs (RENE_SHARD_FRAMES, or any cut in which several ranks add to the same pixel): sum of the
 * [3][yres][xres][4] f32 images onto rank `root`, in place (ncclReduce, ncclSum).  Differs from a one-GPU render only
 * in fp32 summation order. */
int rene_reduce(rene_ctx* ctx, int root);
/* Tile-sharded jobs (RENE_SHARD_TILES: every pixel has exactly one owner): every rank sends ONLY the 32x32 tiles it
 * owns to `root` (1 / n_ranks of the image per rank), which places them; the root's image is then bit-identical to a
 * one-GPU render.  All contexts of the communicator must have been created with shard_count == n_ranks and
 * shard_rank == their rank. */
int rene_gather_tiles(rene_ctx* ctx, int root);

void rene_destroy(rene_ctx* ctx);

/* Validate + flatten + build on the host only (no HIP call): same checks and status codes as
 * rene_create. */
int rene_scene_pack_info(const rene_scene_desc* scene, rene_pack_info* out);

/* The item list the small-scene kernels loop over, as rene_create would upload it (host only, like rene_scene_pack_info): `which` 0 = the
 * main structure, 1 = the emitter structure.  Copies min(cap_items, n) records of 16 floats to `out` (may be NULL with cap_items 0), the loop's
 * items first and the auxiliary records of box items behind them; *n_loop = the loop's items, *n_total (may be NULL) = all records.  Word 15 of a record carries bit 31 where the main item is the emitter structure's only item (the kernels then answer a
 * bounce's emitter query inside the next closest-hit loop; RENE_EMIT_FUSION=0 in the environment marks none).  A scene that does not render
 * through the item loop (no FEAT_SMALL) has no items: *n_loop = 0. */
int rene_scene_small_items(const rene_scene_desc* scene, int which, float* out, uint32_t cap_items, uint32_t* n_loop, uint32_t* n_total);

/* The device memory rene_create would allocate for this scene and these options, without a GPU: RENE_OK for every
 * configuration rene_create accepts (memory permitting), and rene_create's status and message for those it refuses.
 * rene_create allocates by the same plan. */
int rene_plan_memory(const rene_scene_desc* scene, const rene_opts* opts, rene_memory_plan* out);

const char* rene_last_error(void);
uint32_t rene_abi_version(void);

/* ---- output transform (rene/src/main.rs:1758-1810); pure host functions ----------------------- */

/* average (main.rs:1758-1764) then to_rgb8 (main.rs:1785-1792) */
void rene_to_rgb8(const float* sums, size_t n_floats, uint32_t n_samples, uint8_t* out);
/* to_aov / to_aov_normal (main.rs:1794-1810) after average */
void rene_to_aov8(const float* sums, size_t n_floats, uint32_t n_samples, int is_normal, uint8_t* out);
/* The build-defined seed schedule (SURVEY section 8 d): out[k] = frame seed of frame first+k. */
void rene_frame_seeds(uint32_t master_seed, uint32_t first_frame, uint32_t n, uint32_t* out);

/* ---- caller side: pbrt-v3 loader (pbrt-parser/src/lib.rs, rene/src/scene.rs) ------------------ */

typedef struct rene_scene rene_scene;

/* expand_include + parse_pbrt + Scene::create (rene/src/main.rs:107-205). */
int rene_scene_load_pbrt(const char* path, rene_scene** out);
/* same, from memory; base_dir resolves Include / plymesh / imagemap paths */
int rene_scene_parse_pbrt(const char* text, const char* base_dir, rene_scene** out);
const rene_scene_desc* rene_scene_get_desc(const rene_scene* scene);
/* Film filename (intermediate_scene.rs:155-170) */
const char* rene_scene_film_filename(const rene_scene* scene);
/* The name of instance i / material i of the desc's tables, for the Cryptomatte calls; NULL out of range.  An instance made by ObjectInstance "n"
 * is named n -- every shape of the object and every instancing of it -- any other object_<i>; a material of MakeNamedMaterial "n" is named n,
 * any other material_<i> (i: the decimal index into the table). */
const char* rene_scene_instance_name(const rene_scene* scene, uint32_t i);
const char* rene_scene_material_name(const rene_scene* scene, uint32_t i);
void rene_scene_free(rene_scene* scene);

#ifdef __cplusplus
}
#endif
#endif /* RENE_HIP_H */
