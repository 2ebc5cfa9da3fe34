"""ctypes mirror of include/rene_hip.h (one class per C struct, same field order).

This is the binding a Python host uses; INTEGRATION.md shows the equivalent Rust `#[repr(C)]`
declarations.  tests/test_abi.py checks every struct's size against the compiled header.
"""
from __future__ import annotations

import ctypes as C

ABI_VERSION = 7
COMM_ID_BYTES = 128  # RENE_COMM_ID_BYTES (an ncclUniqueId)
DEFAULT_SEED = 0x52454E45
TILE_SIZE = 32
FRAME_STREAM_DEPTHS = 50  # depths per frame of rene_frame_stream_probe (a path ends at depth 50)

# enum mirrors (values = the reference's #[repr(u32)] discriminants, see the header)
SHAPE_TRIANGLE, SHAPE_SPHERE = 0, 1
(MATERIAL_NONE, MATERIAL_MATTE, MATERIAL_GLASS, MATERIAL_SUBSTRATE, MATERIAL_METAL,
 MATERIAL_MIRROR, MATERIAL_UBER, MATERIAL_PLASTIC) = range(8)
TEXTURE_SOLID, TEXTURE_CHECKERBOARD, TEXTURE_IMAGEMAP, TEXTURE_SCALE = range(4)
AREA_LIGHT_NULL, AREA_LIGHT_DIFFUSE = 0, 1
LIGHT_DISTANT = 0
INTEGRATOR_PATH, INTEGRATOR_VOLPATH = 0, 1
LAYER_RADIANCE, LAYER_NORMAL, LAYER_ALBEDO = 0, 1, 2
FLAG_COUNTERS, FLAG_NO_AOV, FLAG_FORCE_BVH, FLAG_SINGLE_LEVEL, FLAG_NO_RESTART, FLAG_DYNAMIC_FIRST, FLAG_WAVEFRONT = 1, 2, 4, 8, 16, 32, 64
FLAG_OVERLAP = 128
FLAG_FP16_PAYLOAD = 256
FLAG_FRAME_GROUPS = 1 << 9
SMALL_ITEM_EMIT_TWIN = 0x80000000  # rene_scene_small_items, word 15 of a main item: it is the emitter structure's only item (csrc/device_scene.h)
FEAT_SMALL = 64  # rene_pack_info.features: the scene renders through the wave-coherent item loop (include/rene_hip.h)
SHARD_TILES, SHARD_FRAMES = 0, 1

STATUS_NAMES = {
    0: "RENE_OK", -1: "RENE_ERR_INVALID_ARGUMENT", -2: "RENE_ERR_INVALID_SCENE",
    -3: "RENE_ERR_DEVICE", -4: "RENE_ERR_UNSUPPORTED", -5: "RENE_ERR_OUT_OF_MEMORY",
    -6: "RENE_ERR_IO", -7: "RENE_ERR_PARSE",
}

f32, u32, i32, u64 = C.c_float, C.c_uint32, C.c_int32, C.c_uint64


class Vertex(C.Structure):
    _fields_ = [("position", f32 * 3), ("normal", f32 * 3), ("uv", f32 * 2)]


class Mesh(C.Structure):
    _fields_ = [("vertices", C.POINTER(Vertex)), ("indices", C.POINTER(u32)),
                ("n_vertices", u32), ("n_indices", u32)]


class Instance(C.Structure):
    _fields_ = [("shape", u32), ("mesh_index", i32), ("material_index", u32),
                ("area_light_index", u32), ("interior_medium_index", u32),
                ("exterior_medium_index", u32), ("matrix", f32 * 12)]


class Material(C.Structure):
    _fields_ = [("type", u32), ("u0", u32 * 4), ("u1", u32 * 4), ("v0", f32 * 4)]


class Texture(C.Structure):
    _fields_ = [("type", u32), ("u0", u32 * 4), ("v0", f32 * 4)]


class AreaLight(C.Structure):
    _fields_ = [("type", u32), ("v0", f32 * 4)]


class Light(C.Structure):
    _fields_ = [("type", u32), ("v0", f32 * 4), ("v1", f32 * 4)]


MEDIUM_VACUUM, MEDIUM_HOMOGENEOUS = 0, 1


class Medium(C.Structure):
    _fields_ = [("type", u32), ("v0", f32 * 4), ("v1", f32 * 4)]


class Image(C.Structure):
    _fields_ = [("rgba", C.POINTER(f32)), ("width", u32), ("height", u32)]


class Uniform(C.Structure):
    _fields_ = [("camera_to_world", f32 * 16), ("background_matrix", f32 * 16),
                ("background_color", f32 * 4), ("projection_inv", f32 * 16),
                ("background_texture", u32)]


class SceneDesc(C.Structure):
    _fields_ = [("struct_size", u32), ("integrator", u32), ("xresolution", u32),
                ("yresolution", u32), ("uniform", Uniform),
                ("n_instances", u32), ("n_meshes", u32), ("n_materials", u32),
                ("n_textures", u32), ("n_area_lights", u32), ("n_lights", u32),
                ("n_images", u32),
                ("instances", C.POINTER(Instance)), ("meshes", C.POINTER(Mesh)),
                ("materials", C.POINTER(Material)), ("textures", C.POINTER(Texture)),
                ("area_lights", C.POINTER(AreaLight)), ("lights", C.POINTER(Light)),
                ("images", C.POINTER(Image)), ("mediums", C.POINTER(Medium)), ("n_mediums", u32),
                ("reserved", u32)]


class Opts(C.Structure):
    _fields_ = [("struct_size", u32), ("seed", u32), ("device", i32), ("flags", u32),
                ("shard_mode", u32), ("shard_rank", u32), ("shard_count", u32),
                ("reserved", u32), ("framebuffer", C.c_void_p), ("stream", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("rays_closest", u64), ("rays_shadow", u64), ("rays_emitter", u64),
                ("paths", u64), ("bounces", u64), ("hits", u64), ("adds", u64),
                ("node_visits", u64), ("prim_tests", u64), ("frames", u64), ("launches", u64),
                ("kernel_ms", C.c_double), ("last_launch_ms", C.c_double), ("sclk_mhz", C.c_double)]

    @property
    def rays(self) -> int:
        return self.rays_closest + self.rays_shadow + self.rays_emitter

    def as_dict(self) -> dict:
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["rays"] = self.rays
        return d


class PackInfo(C.Structure):
    _fields_ = [("n_instances", u32), ("n_triangles", u32), ("n_spheres", u32),
                ("n_nodes_main", u32), ("n_slots_main", u32), ("depth_main", u32),
                ("n_nodes_emit", u32), ("n_slots_emit", u32), ("depth_emit", u32),
                ("features", u32), ("emit_object_len", u32), ("lights_len", u32),
                ("device_bytes", u64), ("n_items_main", u32), ("n_items_emit", u32)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class MemoryPlan(C.Structure):
    """rene_memory_plan: the device memory rene_create allocates for a scene and options (bytes)."""
    _fields_ = [("chain_bytes", u64), ("version_bytes", u64), ("image_bytes", u64), ("scene_bytes", u64),
                ("queue_bytes", u64), ("total_bytes", u64)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class DenoiseParams(C.Structure):
    """rene_denoise_params: the constants of the `atrous` denoiser (rene_denoise_params_default fills the defaults)."""
    _fields_ = [("struct_size", u32), ("iterations", u32), ("sigma_luminance", f32), ("sigma_normal2", f32),
                ("sigma_albedo2", f32), ("albedo_floor", f32), ("relative_floor", f32), ("reserved", u32)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


DENOISED_RADIANCE, DENOISED_VARIANCE, DENOISED_MEAN, DENOISED_TRIM = 0, 1, 2, 3
DENOISE_BYTES_PER_PIXEL = 84


class DenoiseShardHeader(C.Structure):
    """rene_denoise_shard_header: what a tile shard's packed denoise buffer starts with (rene_denoise_shard_prepare)."""
    _fields_ = [("magic", u32), ("header_bytes", u32), ("width", u32), ("height", u32), ("shard_rank", u32), ("shard_count", u32),
                ("n_owned", u32), ("reserved", u32), ("params", DenoiseParams)]


class DenoiseShardTile(C.Structure):
    """rene_denoise_shard_tile: one owned tile's entry of the table behind the header -- its frame count and whether it takes part in the filter."""
    _fields_ = [("n_frames", u32), ("valid", u32)]


DENOISE_SHARD_TILE_DTYPE = [("n_frames", "<u4"), ("valid", "<u4")]
DENOISE_SHARD_MAGIC = 0x48534E44
DENOISE_SHARD_TILE_BYTES = 53248  # rec [1024][4], guides [1024][2][4], var [1024] floats: 52 bytes per slot


class NoiseParams(C.Structure):
    """rene_noise_params: the constant of the noise estimate (rene_noise_params_default fills the default)."""
    _fields_ = [("struct_size", u32), ("reserved0", u32), ("luminance_floor", f32), ("reserved1", u32)]


class NoiseTile(C.Structure):
    """rene_noise_tile: one 32 x 32 tile's record -- the sums of its pixels' variance of the mean and luminance, its pixels inside the image."""
    _fields_ = [("sum_var", f32), ("sum_lum", f32), ("n_pixels", u32), ("reserved", u32)]


NOISE_TILE_DTYPE = [("sum_var", "<f4"), ("sum_lum", "<f4"), ("n_pixels", "<u4"), ("reserved", "<u4")]


class NoiseEstimate(C.Structure):
    """rene_noise_estimate: the additive fields of a context's (or tile shard's) estimate and the figures derived from them."""
    _fields_ = [("struct_size", u32), ("n_tiles", u32), ("n_pixels", u64), ("sum_var", C.c_double), ("sum_lum", C.c_double),
                ("sum_weighted_q", C.c_double), ("n_frames", u64), ("n_chains", u32), ("luminance_floor", f32),
                ("noise", C.c_double), ("rel_rmse", C.c_double), ("worst_tile_noise", C.c_double), ("worst_tile", u32), ("reserved", u32)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class RobustParams(C.Structure):
    """rene_robust_params: the constants of the firefly-robust resolve (rene_robust_params_default fills the defaults)."""
    _fields_ = [("struct_size", u32), ("max_trim", u32), ("gain", f32), ("reserved", u32)]


class RobustTile(C.Structure):
    """rene_robust_tile: one 32 x 32 tile's record -- the sums of the plain and of the robust mean's luminance, its pixels inside the image, those trimmed."""
    _fields_ = [("sum_lum_plain", f32), ("sum_lum_robust", f32), ("n_pixels", u32), ("n_trimmed", u32)]


ROBUST_TILE_DTYPE = [("sum_lum_plain", "<f4"), ("sum_lum_robust", "<f4"), ("n_pixels", "<u4"), ("n_trimmed", "<u4")]
ROBUST_IMAGE, ROBUST_TRIM = 0, 1


class RobustSummary(C.Structure):
    """rene_robust_summary: the additive fields of a context's (or tile shard's) resolve and the energy kept, derived from them."""
    _fields_ = [("struct_size", u32), ("n_tiles", u32), ("n_pixels", u64), ("n_trimmed", u64), ("sum_lum_plain", C.c_double),
                ("sum_lum_robust", C.c_double), ("kept_energy", C.c_double), ("n_frames", u64), ("max_trim", u32), ("gain", f32)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class FeatureParams(C.Structure):
    """rene_feature_params: which features rene_export_features writes, in which element format and layout (rene_feature_params_default fills the defaults)."""
    _fields_ = [("struct_size", u32), ("features", u32), ("format", u32), ("layout", u32)]


FEATURE_COLOR, FEATURE_ALBEDO, FEATURE_NORMAL, FEATURE_VARIANCE, FEATURE_HALF_A, FEATURE_HALF_B, FEATURE_FRAMES = (1 << _b for _b in range(7))
FEATURE_DEFAULT = FEATURE_COLOR | FEATURE_ALBEDO | FEATURE_NORMAL
FEATURE_ALL = 127
FEATURES_F32, FEATURES_F16 = 0, 1
FEATURES_CHW, FEATURES_HWC = 0, 1


class OutputParams(C.Structure):
    """rene_output_params: which image rene_output_8bit transforms and into which pixel format (rene_output_params_default fills the defaults)."""
    _fields_ = [("struct_size", u32), ("source", u32), ("format", u32), ("reserved", u32)]


OUTPUT_RADIANCE, OUTPUT_NORMAL, OUTPUT_ALBEDO, OUTPUT_DENOISED, OUTPUT_DENOISED_MEAN, OUTPUT_ROBUST = range(6)
OUTPUT_RGB8, OUTPUT_RGBA8 = 0, 1
OUTPUT_SRGB, OUTPUT_AOV, OUTPUT_AOV_NORMAL = 0, 1, 2


class TonemapParams(C.Structure):
    """rene_tonemap_params: rene_output_tonemapped's image, pixel format, operator, exposure factor and white point (rene_tonemap_params_default
    fills the defaults)."""
    _fields_ = [("struct_size", u32), ("source", u32), ("format", u32), ("op", u32), ("scale", f32), ("white", f32), ("reserved", u32 * 2)]


TONEMAP_CLAMP, TONEMAP_REINHARD, TONEMAP_ACES = 0, 1, 2
EXPOSURE_KEY_E8, EXPOSURE_E8_MIN, EXPOSURE_E8_MAX = -20, -960, 960
LUMINANCE_BINS = 256


class LuminanceStats(C.Structure):
    """rene_luminance_stats: the luminance histogram of an image (or of a tile shard's part of it)."""
    _fields_ = [("struct_size", u32), ("counts", u32 * LUMINANCE_BINS), ("n_dark", u32), ("n_pixels", u32)]


STATE_MAGIC = 0x54534E52  # "RNST"
STATE_VERSION = 1
STATE_HEADER_BYTES = 256
STATE_TILE_BYTES = 294912  # [8 chains][3 layers][32 dy][32 dx][3] float32
STATE_TILE_ACTIVE = 1


class StateHeader(C.Structure):
    """rene_state_header: the 256 bytes a saved state (one part) starts with."""
    _fields_ = [("magic", u32), ("version", u32), ("header_bytes", u32), ("tile_size", u32), ("width", u32), ("height", u32), ("tiles_x", u32),
                ("tiles_y", u32), ("seed", u32), ("frame_base", u32), ("n_frames", u32), ("frames_contiguous", u32), ("loaded", u32), ("n_tiles", u32),
                ("paths", u64), ("chain_frames", u64 * 8), ("fingerprint", u64 * 2), ("payload_offset", u64), ("total_bytes", u64),
                ("reserved", C.c_uint8 * 96)]


class StateTile(C.Structure):
    """rene_state_tile: one tile's entry of a part's table -- its index on the full grid, N_t, flags and the checksum of its payload."""
    _fields_ = [("tile", u32), ("n_frames", u32), ("flags", u32), ("c0", u32), ("c1", u32), ("reserved", u32 * 3)]


STATE_TILE_DTYPE = [("tile", "<u4"), ("n_frames", "<u4"), ("flags", "<u4"), ("c0", "<u4"), ("c1", "<u4"), ("reserved", "<u4", (3,))]


class StateInfo(C.Structure):
    """rene_state_info: what rene_state_inspect reads from a part's header."""
    _fields_ = [("struct_size", u32), ("version", u32), ("width", u32), ("height", u32), ("tile_size", u32), ("tiles_x", u32), ("tiles_y", u32),
                ("seed", u32), ("frame_base", u32), ("n_frames", u32), ("frames_contiguous", u32), ("loaded", u32), ("n_tiles", u32), ("reserved", u32),
                ("paths", u64), ("chain_frames", u64 * 8), ("fingerprint", u64 * 2), ("payload_offset", u64), ("total_bytes", u64)]

    def as_dict(self) -> dict:
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["chain_frames"] = list(self.chain_frames)
        d["fingerprint"] = tuple(self.fingerprint)
        return d


class StateParams(C.Structure):
    """rene_state_params: the chunking of rene_save_state / rene_restore_state (rene_state_params_default fills the default)."""
    _fields_ = [("struct_size", u32), ("chunk_tiles", u32), ("reserved", u32 * 2)]


class Hit(C.Structure):
    _fields_ = [("t", f32), ("u", f32), ("v", f32), ("instance", u32), ("primitive", u32)]


class GbufferParams(C.Structure):
    """rene_gbuffer_params: the frames and the id source of the geometry pass (rene_gbuffer_params_default fills the defaults)."""
    _fields_ = [("struct_size", u32), ("first_frame", u32), ("n_frames", u32), ("id_source", u32), ("flags", u32)]


class GbufferPixel(C.Structure):
    """rene_gbuffer_pixel: one pixel's record of the geometry pass, 64 bytes."""
    _fields_ = [("depth_sum", f32), ("depth_min", f32), ("hits", u32), ("n", u32), ("position_sum", f32 * 3), ("other", u32),
                ("id", u32 * 4), ("count", u32 * 4)]


class PrimaryHit(C.Structure):
    """rene_primary_hit: one sample of the geometry pass, 32 bytes."""
    _fields_ = [("d", f32 * 3), ("t", f32), ("u", f32), ("v", f32), ("instance", u32), ("primitive", u32)]


GBUFFER_ID_INSTANCE, GBUFFER_ID_MATERIAL, GBUFFER_ID_PRIMITIVE = 0, 1, 2
GBUFFER_MAX_FRAMES = 65536
GBUFFER_ID_NONE = 0xFFFFFFFF
GBUFFER_DTYPE = [("depth_sum", "<f4"), ("depth_min", "<f4"), ("hits", "<u4"), ("n", "<u4"), ("position_sum", "<f4", (3,)), ("other", "<u4"),
                 ("id", "<u4", (4,)), ("count", "<u4", (4,))]
PRIMARY_HIT_DTYPE = [("d", "<f4", (3,)), ("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("instance", "<u4"), ("primitive", "<u4")]


class OcclusionParams(C.Structure):
    """rene_occlusion_params: the frames, the rays per hitting sample and their radius (rene_occlusion_params_default fills the defaults)."""
    _fields_ = [("struct_size", u32), ("first_frame", u32), ("n_frames", u32), ("rays", u32), ("radius", f32), ("flags", u32)]


class OcclusionPixel(C.Structure):
    """rene_occlusion_pixel: one pixel's record of the occlusion pass, 32 bytes."""
    _fields_ = [("hits", u32), ("rays", u32), ("occluded", u32), ("n", u32), ("bent_sum", f32 * 3), ("reserved", u32)]


class OcclusionSample(C.Structure):
    """rene_occlusion_sample: one occlusion ray of the pass, 48 bytes."""
    _fields_ = [("p", f32 * 3), ("state", u32), ("n", f32 * 3), ("r1", f32), ("w", f32 * 3), ("r2", f32)]


OCCLUSION_MAX_RAYS = 64
OCCLUSION_MAX_FRAMES = 65536
OCCLUSION_MISS, OCCLUSION_OPEN, OCCLUSION_OCCLUDED, OCCLUSION_NO_RAY = 0, 1, 2, 3
OCCLUSION_DTYPE = [("hits", "<u4"), ("rays", "<u4"), ("occluded", "<u4"), ("n", "<u4"), ("bent_sum", "<f4", (3,)), ("reserved", "<u4")]
OCCLUSION_SAMPLE_DTYPE = [("p", "<f4", (3,)), ("state", "<u4"), ("n", "<f4", (3,)), ("r1", "<f4"), ("w", "<f4", (3,)), ("r2", "<f4")]


class DirectParams(C.Structure):
    """rene_direct_params: the frames of the direct-light pass (rene_direct_params_default fills the defaults)."""
    _fields_ = [("struct_size", u32), ("first_frame", u32), ("n_frames", u32), ("flags", u32)]


class DirectPixel(C.Structure):
    """rene_direct_pixel: one pixel's record of the direct-light pass, 48 bytes."""
    _fields_ = [("seen", f32 * 3), ("hits", u32), ("distant", f32 * 3), ("n", u32), ("sampled", f32 * 3), ("reserved", u32)]


class DirectSample(C.Structure):
    """rene_direct_sample: one sample of the direct-light pass, 64 bytes."""
    _fields_ = [("seen", f32 * 3), ("state", u32), ("distant", f32 * 3), ("pdf", f32), ("wi", f32 * 3), ("second", u32), ("sampled", f32 * 3),
                ("reserved", u32)]


DIRECT_MAX_FRAMES = 65536
DIRECT_MISS, DIRECT_LIGHT, DIRECT_BSDF, DIRECT_PLAIN, DIRECT_ENDED_PDF, DIRECT_ENDED_ZERO = 0, 1, 2, 3, 4, 5
DIRECT_SECOND_NONE, DIRECT_SECOND_MISS, DIRECT_SECOND_SURFACE, DIRECT_SECOND_EMITTER = 0, 1, 2, 3
DIRECT_DTYPE = [("seen", "<f4", (3,)), ("hits", "<u4"), ("distant", "<f4", (3,)), ("n", "<u4"), ("sampled", "<f4", (3,)), ("reserved", "<u4")]
DIRECT_SAMPLE_DTYPE = [("seen", "<f4", (3,)), ("state", "<u4"), ("distant", "<f4", (3,)), ("pdf", "<f4"), ("wi", "<f4", (3,)), ("second", "<u4"),
                       ("sampled", "<f4", (3,)), ("reserved", "<u4")]


class BouncesParams(C.Structure):
    """rene_bounces_params: the frames of the bounce pass and the cap on a path's iterations (rene_bounces_params_default fills the defaults)."""
    _fields_ = [("struct_size", u32), ("first_frame", u32), ("n_frames", u32), ("max_depth", u32), ("flags", u32)]


class BouncesBucket(C.Structure):
    """rene_bounces_bucket: what one iteration of the path loop added (bucket 9: every iteration from 9 on), and how often it was reached."""
    _fields_ = [("sum", f32 * 3), ("reached", u32)]


class BouncesPixel(C.Structure):
    """rene_bounces_pixel: one pixel's record of the bounce pass, 176 bytes."""
    _fields_ = [("bucket", BouncesBucket * 10), ("n", u32), ("length_sum", u32), ("length_max", u32), ("capped", u32)]


class BouncesSample(C.Structure):
    """rene_bounces_sample: one sample of the bounce pass, 176 bytes."""
    _fields_ = [("bucket", BouncesBucket * 10), ("n", u32), ("length", u32), ("end", u32), ("reserved", u32)]


BOUNCES_MAX_FRAMES = 65536
BOUNCES_BUCKETS = 10
BOUNCES_MAX_DEPTH = 50
BOUNCES_END_MISS, BOUNCES_END_PDF, BOUNCES_END_ZERO, BOUNCES_END_ROULETTE, BOUNCES_END_CAP = 0, 1, 2, 3, 4
BOUNCES_BUCKET_DTYPE = [("sum", "<f4", (3,)), ("reached", "<u4")]
BOUNCES_DTYPE = [("bucket", BOUNCES_BUCKET_DTYPE, (10,)), ("n", "<u4"), ("length_sum", "<u4"), ("length_max", "<u4"), ("capped", "<u4")]
BOUNCES_SAMPLE_DTYPE = [("bucket", BOUNCES_BUCKET_DTYPE, (10,)), ("n", "<u4"), ("length", "<u4"), ("end", "<u4"), ("reserved", "<u4")]


class LightsParams(C.Structure):
    """rene_lights_params: the frames of the light-group pass and the caller's grouping -- host pointers to one uint8 group per instance and per
    distant light, and the background's group (rene_lights_params_default fills the defaults: no tables, the library's own grouping)."""
    _fields_ = [("struct_size", u32), ("first_frame", u32), ("n_frames", u32), ("flags", u32), ("n_instances", u32), ("n_distant", u32),
                ("instance_group", C.c_void_p), ("distant_group", C.c_void_p), ("background_group", C.c_uint8)]


class LightsGroup(C.Structure):
    """rene_lights_group: what the sources of one group added, and how many of the adds were not black."""
    _fields_ = [("sum", f32 * 3), ("adds", u32)]


class LightsPixel(C.Structure):
    """rene_lights_pixel: one pixel's record of the light-group pass, 144 bytes."""
    _fields_ = [("group", LightsGroup * 8), ("n", u32), ("lit", u32), ("reserved", u32 * 2)]


class LightsSample(C.Structure):
    """rene_lights_sample: one sample of the light-group pass, 144 bytes."""
    _fields_ = [("group", LightsGroup * 8), ("n", u32), ("lit", u32), ("length", u32), ("end", u32)]


LIGHTS_MAX_FRAMES = 65536
LIGHTS_GROUPS = 8
LIGHTS_GROUP_DTYPE = [("sum", "<f4", (3,)), ("adds", "<u4")]
LIGHTS_DTYPE = [("group", LIGHTS_GROUP_DTYPE, (8,)), ("n", "<u4"), ("lit", "<u4"), ("reserved", "<u4", (2,))]
LIGHTS_SAMPLE_DTYPE = [("group", LIGHTS_GROUP_DTYPE, (8,)), ("n", "<u4"), ("lit", "<u4"), ("length", "<u4"), ("end", "<u4")]


class ExrParams(C.Structure):
    """rene_exr_params: which layers rene_output_exr packs and which image its R G B are (rene_exr_params_default fills the defaults)."""
    _fields_ = [("struct_size", u32), ("layers", u32), ("beauty_source", u32), ("reserved", u32)]


class ExrPlanes(C.Structure):
    """rene_exr_planes: the planes of means rene_exr_body_host packs, host pointers (a plane whose layer is not chosen may be NULL)."""
    _fields_ = [("struct_size", u32), ("reserved", u32), ("beauty", C.c_void_p), ("albedo", C.c_void_p), ("normal", C.c_void_p), ("denoised", C.c_void_p),
                ("alpha", C.c_void_p), ("depth", C.c_void_p), ("position", C.c_void_p), ("ids", C.c_void_p), ("coverage", C.c_void_p)]


EXR_BEAUTY, EXR_ALBEDO, EXR_NORMAL, EXR_DENOISED, EXR_ALPHA, EXR_DEPTH, EXR_POSITION, EXR_IDS = (1 << _b for _b in range(8))
EXR_DEFAULT = EXR_BEAUTY | EXR_ALBEDO | EXR_NORMAL
EXR_ALL = 255
EXR_MAX_SIZE = 16384
EXR_COMPRESSION_NONE, EXR_COMPRESSION_ZIPS = 0, 2  # the file format's own codes (rene_exr_compress)
# every channel a file can hold, in file order (the order of the names' bytes): name, layer bit, pixel type
EXR_CHANNELS = [
    ("A", EXR_ALPHA, "half"), ("B", EXR_BEAUTY, "half"), ("G", EXR_BEAUTY, "half"), ("P.X", EXR_POSITION, "float"), ("P.Y", EXR_POSITION, "float"),
    ("P.Z", EXR_POSITION, "float"), ("R", EXR_BEAUTY, "half"), ("Z", EXR_DEPTH, "float"), ("albedo.B", EXR_ALBEDO, "half"), ("albedo.G", EXR_ALBEDO, "half"),
    ("albedo.R", EXR_ALBEDO, "half"), ("cov0", EXR_IDS, "half"), ("cov1", EXR_IDS, "half"), ("cov2", EXR_IDS, "half"), ("cov3", EXR_IDS, "half"),
    ("denoised.B", EXR_DENOISED, "half"), ("denoised.G", EXR_DENOISED, "half"), ("denoised.R", EXR_DENOISED, "half"), ("id0", EXR_IDS, "uint"),
    ("id1", EXR_IDS, "uint"), ("id2", EXR_IDS, "uint"), ("id3", EXR_IDS, "uint"), ("normal.X", EXR_NORMAL, "half"), ("normal.Y", EXR_NORMAL, "half"),
    ("normal.Z", EXR_NORMAL, "half"),
]

CRYPTOMATTE_MAX_LAYERS = 3
CRYPTOMATTE_MAX_NAME = 24


class CryptomatteLayer(C.Structure):
    """rene_cryptomatte_layer: a layer's name, which ids its records hold, the name of every id and the records (a device pointer, or NULL: the
    library-owned result of the last rene_gbuffer)."""
    _fields_ = [("name", C.c_char_p), ("id_source", u32), ("n_names", u32), ("names", C.POINTER(C.c_char_p)), ("records", C.c_void_p)]


class CryptomatteParams(C.Structure):
    """rene_cryptomatte_params: the layers rene_output_cryptomatte packs."""
    _fields_ = [("struct_size", u32), ("n_layers", u32), ("layers", C.POINTER(CryptomatteLayer)), ("reserved", C.c_uint64)]

EXRP_AO, EXRP_BENT, EXRP_BOUNCES, EXRP_DIRECT, EXRP_INDIRECT, EXRP_LIGHTS, EXRP_LENGTH = (1 << _b for _b in range(7))
EXRP_ALL = 127
EXRP_MAX_NAME = 24


class ExrPassesParams(C.Structure):
    """rene_exr_passes_params: the pass layers of rene_output_exr_passes, the light groups it writes and their names, and the four record sources
    (device pointers, or NULL: the library-owned result of the pass; host pointers for rene_exr_passes_body_host)."""
    _fields_ = [("struct_size", u32), ("layers", u32), ("groups", u32), ("reserved", u32), ("group_names", C.POINTER(C.c_char_p)),
                ("occlusion", C.c_void_p), ("direct", C.c_void_p), ("bounces", C.c_void_p), ("lights", C.c_void_p)]


def algorithmic_bytes(stats) -> int:
    """cache-less traffic model,
    B_alg = 64 N_ray + 64 N_node + 48 N_tri + 144 N_hit + 128 N_bounce + 32 N_add."""
    g = (lambda k: stats[k]) if isinstance(stats, dict) else (lambda k: getattr(stats, k))
    n_ray = g("rays_closest") + g("rays_shadow") + g("rays_emitter")
    return (64 * n_ray + 64 * g("node_visits") + 48 * g("prim_tests") + 144 * g("hits")
            + 128 * g("bounces") + 32 * g("adds"))


# every symbol include/rene_hip.h declares (tests check that the shared library exports them all)
EXPORTED_SYMBOLS = [
    "rene_create", "rene_render", "rene_sync", "rene_download", "rene_reset", "rene_tune", "rene_framebuffer",
    "rene_get_stats", "rene_denoise_params_default", "rene_denoise", "rene_denoise_tiles", "rene_download_denoised", "rene_denoised_buffer",
    "rene_noise_params_default", "rene_estimate_noise", "rene_download_noise_tiles", "rene_noise_combine", "rene_noise_frames_needed",
    "rene_set_active_tiles", "rene_tile_frames", "rene_download_mean", "rene_noise_select_tiles",
    "rene_robust_params_default", "rene_resolve_robust", "rene_download_robust", "rene_download_robust_tiles", "rene_robust_combine",
    "rene_denoise_robust_params_default", "rene_denoise_robust", "rene_denoise_tiles_robust",
    "rene_denoise_shard_bytes", "rene_denoise_shard_prepare", "rene_denoise_shard_buffer", "rene_download_denoise_shard",
    "rene_denoise_place_shard", "rene_denoise_placed", "rene_gather_denoise",
    "rene_feature_params_default", "rene_feature_channels", "rene_export_features", "rene_features_buffer", "rene_download_features",
    "rene_output_params_default", "rene_output_8bit", "rene_output_buffer", "rene_download_output", "rene_output_thresholds", "rene_output_probe",
    "rene_tonemap_params_default", "rene_output_tonemapped", "rene_luminance_histogram", "rene_luminance_combine", "rene_luminance_mean_bin_x256",
    "rene_luminance_percentile_bin", "rene_auto_exposure_e8", "rene_exposure_scale", "rene_tonemap_rgb8", "rene_luminance_histogram_host",
    "rene_tonemap_probe",
    "rene_gbuffer_params_default", "rene_gbuffer_bytes", "rene_gbuffer", "rene_gbuffer_buffer", "rene_download_gbuffer", "rene_primary_hits",
    "rene_occlusion_params_default", "rene_occlusion_bytes", "rene_occlusion", "rene_occlusion_buffer", "rene_download_occlusion", "rene_occlusion_samples",
    "rene_direct_params_default", "rene_direct_bytes", "rene_direct", "rene_direct_buffer", "rene_download_direct", "rene_direct_samples",
    "rene_bounces_params_default", "rene_bounces_bytes", "rene_bounces", "rene_bounces_buffer", "rene_download_bounces", "rene_bounces_samples",
    "rene_lights_params_default", "rene_lights_bytes", "rene_lights_default_groups", "rene_lights", "rene_lights_buffer", "rene_download_lights",
    "rene_lights_samples",
    "rene_exr_params_default", "rene_exr_layout", "rene_exr_header", "rene_output_exr", "rene_exr_buffer", "rene_download_exr", "rene_write_exr",
    "rene_exr_body_host",
    "rene_exr_tail_bound", "rene_exr_attributes", "rene_exr_compress_host", "rene_exr_compress", "rene_exr_tail_buffer", "rene_download_exr_tail",
    "rene_output_exr_compressed", "rene_write_exr_compressed", "rene_exr_compress_rows_host", "rene_exr_compress_rows",
    "rene_cryptomatte_params_default", "rene_cryptomatte_hash", "rene_cryptomatte_manifest", "rene_cryptomatte_layout", "rene_cryptomatte_attributes",
    "rene_cryptomatte_body_host", "rene_output_cryptomatte", "rene_cryptomatte_buffer", "rene_download_cryptomatte", "rene_write_cryptomatte",
    "rene_exr_passes_params_default", "rene_exr_passes_layout", "rene_exr_passes_attributes", "rene_exr_passes_body_host", "rene_output_exr_passes",
    "rene_exr_passes_buffer", "rene_download_exr_passes", "rene_write_exr_passes",
    "rene_state_params_default", "rene_scene_fingerprint", "rene_state_bytes", "rene_save_state", "rene_restore_state", "rene_state_inspect",
    "rene_state_tiles", "rene_state_verify", "rene_state_inspect_file", "rene_save_state_file", "rene_restore_state_files",
    "rene_trace", "rene_ray_dump", "rene_trace_queue", "rene_bsdf_eval", "rene_medium_eval", "rene_transmittance", "rene_emitter_pdf", "rene_emitter_pdf_form", "rene_emit_sample", "rene_pcg_probe", "rene_frame_stream_probe", "rene_load_chains",
    "rene_comm_unique_id", "rene_comm_init", "rene_comm_init_all", "rene_comm_group_begin", "rene_comm_group_end",
    "rene_reduce", "rene_gather_tiles", "rene_destroy", "rene_scene_pack_info", "rene_scene_small_items", "rene_plan_memory", "rene_last_error", "rene_abi_version",
    "rene_to_rgb8", "rene_to_aov8", "rene_frame_seeds",
    "rene_scene_load_pbrt", "rene_scene_parse_pbrt", "rene_scene_get_desc",
    "rene_scene_film_filename", "rene_scene_instance_name", "rene_scene_material_name", "rene_scene_free",
]
