"""Python host binding of librene_hip.so (the C ABI of include/rene_hip.h).

The render path has NO CPU fallback: if the HIP library is missing or no GPU is visible, every
entry point raises.  (The CPU restatement under oracle/ is test infrastructure and is never
imported from here.)
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from . import abi

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
# RENE_HIP_LIB names another build of the same library in csrc/ (A/B measurements of kernel variants, Makefile `variant`)
LIB_PATH = os.path.join(_CSRC, os.environ.get("RENE_HIP_LIB", "librene_hip.so"))
_LIB = None


class ReneError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"{abi.STATUS_NAMES.get(code, code)}: {message}")
        self.code = code


def build(force: bool = False) -> str:
    """Compile the HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", _CSRC, "-j4"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ReneError(-3, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(there is no CPU fallback for the render path)")
    # PyTorch bundles its own libamdhip64.so.7; whichever copy is loaded first serves the whole
    # process.  Load torch's first (when torch is installed) so that device pointers and streams can
    # be shared with torch tensors / torch.distributed (bench.py, multi-GPU reduce).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
    L.rene_create.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.Opts), C.POINTER(vp)]
    L.rene_render.argtypes = [vp, u32, u32]
    L.rene_sync.argtypes = [vp]
    L.rene_download.argtypes = [vp, i32, i32, vp, C.c_size_t]
    L.rene_reset.argtypes = [vp]
    L.rene_tune.argtypes = [vp, C.c_uint32]
    L.rene_framebuffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rene_get_stats.argtypes = [vp, C.POINTER(abi.Stats)]
    L.rene_denoise_params_default.argtypes = [C.POINTER(abi.DenoiseParams)]
    L.rene_denoise_params_default.restype = None
    L.rene_denoise.argtypes = [vp, C.POINTER(abi.DenoiseParams)]
    L.rene_denoise_tiles.argtypes = [vp, C.POINTER(abi.DenoiseParams)]
    L.rene_download_denoised.argtypes = [vp, i32, i32, vp, C.c_size_t]
    L.rene_denoised_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rene_noise_params_default.argtypes = [C.POINTER(abi.NoiseParams)]
    L.rene_noise_params_default.restype = None
    L.rene_estimate_noise.argtypes = [vp, C.POINTER(abi.NoiseParams), C.POINTER(abi.NoiseEstimate)]
    L.rene_download_noise_tiles.argtypes = [vp, vp, C.c_size_t]
    L.rene_noise_combine.argtypes = [C.POINTER(abi.NoiseEstimate), C.c_size_t, C.POINTER(abi.NoiseEstimate)]
    L.rene_noise_frames_needed.argtypes = [C.POINTER(abi.NoiseEstimate), C.c_double]
    L.rene_noise_frames_needed.restype = u32
    L.rene_set_active_tiles.argtypes = [vp, vp, C.c_size_t]
    L.rene_tile_frames.argtypes = [vp, vp, C.c_size_t]
    L.rene_download_mean.argtypes = [vp, i32, i32, vp, C.c_size_t]
    L.rene_noise_select_tiles.argtypes = [vp, vp, u32, u32, C.c_float, C.c_double, u32, vp]
    L.rene_robust_params_default.argtypes = [C.POINTER(abi.RobustParams)]
    L.rene_robust_params_default.restype = None
    L.rene_resolve_robust.argtypes = [vp, C.POINTER(abi.RobustParams), C.POINTER(abi.RobustSummary)]
    L.rene_download_robust.argtypes = [vp, i32, i32, vp, C.c_size_t]
    L.rene_download_robust_tiles.argtypes = [vp, vp, C.c_size_t]
    L.rene_robust_combine.argtypes = [C.POINTER(abi.RobustSummary), C.c_size_t, C.POINTER(abi.RobustSummary)]
    L.rene_denoise_robust_params_default.argtypes = [C.POINTER(abi.RobustParams)]
    L.rene_denoise_robust_params_default.restype = None
    L.rene_denoise_robust.argtypes = [vp, C.POINTER(abi.DenoiseParams), C.POINTER(abi.RobustParams)]
    L.rene_denoise_tiles_robust.argtypes = [vp, C.POINTER(abi.DenoiseParams), C.POINTER(abi.RobustParams)]
    L.rene_denoise_shard_bytes.argtypes = [u32, u32, u32, u32]
    L.rene_denoise_shard_bytes.restype = C.c_size_t
    L.rene_denoise_shard_prepare.argtypes = [vp, C.POINTER(abi.DenoiseParams)]
    L.rene_denoise_shard_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rene_download_denoise_shard.argtypes = [vp, vp, C.c_size_t]
    L.rene_denoise_place_shard.argtypes = [vp, vp, C.c_size_t]
    L.rene_denoise_placed.argtypes = [vp]
    L.rene_gather_denoise.argtypes = [vp, i32]
    L.rene_feature_params_default.argtypes = [C.POINTER(abi.FeatureParams)]
    L.rene_feature_params_default.restype = None
    L.rene_feature_channels.argtypes = [u32]
    L.rene_feature_channels.restype = u32
    L.rene_export_features.argtypes = [vp, C.POINTER(abi.FeatureParams), vp, C.c_size_t]
    L.rene_features_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rene_download_features.argtypes = [vp, vp, C.c_size_t]
    L.rene_output_params_default.argtypes = [C.POINTER(abi.OutputParams)]
    L.rene_output_params_default.restype = None
    L.rene_output_8bit.argtypes = [vp, C.POINTER(abi.OutputParams), vp, C.c_size_t]
    L.rene_output_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rene_download_output.argtypes = [vp, vp, C.c_size_t]
    L.rene_output_thresholds.argtypes = [vp]
    L.rene_output_thresholds.restype = None
    L.rene_output_probe.argtypes = [i32, i32, C.c_size_t, vp, vp]
    L.rene_tonemap_params_default.argtypes = [C.POINTER(abi.TonemapParams)]
    L.rene_tonemap_params_default.restype = None
    L.rene_output_tonemapped.argtypes = [vp, C.POINTER(abi.TonemapParams), vp, C.c_size_t]
    L.rene_luminance_histogram.argtypes = [vp, u32, C.POINTER(abi.LuminanceStats)]
    L.rene_luminance_combine.argtypes = [C.POINTER(abi.LuminanceStats), C.c_size_t, C.POINTER(abi.LuminanceStats)]
    L.rene_luminance_mean_bin_x256.argtypes = [C.POINTER(abi.LuminanceStats)]
    L.rene_luminance_mean_bin_x256.restype = u32
    L.rene_luminance_percentile_bin.argtypes = [C.POINTER(abi.LuminanceStats), u32]
    L.rene_auto_exposure_e8.argtypes = [C.POINTER(abi.LuminanceStats), i32]
    L.rene_exposure_scale.argtypes = [i32]
    L.rene_exposure_scale.restype = C.c_float
    L.rene_tonemap_rgb8.argtypes = [vp, C.c_size_t, i32, u32, C.c_float, C.c_float, vp]
    L.rene_luminance_histogram_host.argtypes = [vp, C.c_size_t, i32, C.POINTER(abi.LuminanceStats)]
    L.rene_tonemap_probe.argtypes = [i32, u32, C.c_float, C.c_float, C.c_size_t, vp, vp]
    L.rene_gbuffer_params_default.argtypes = [C.POINTER(abi.GbufferParams)]
    L.rene_gbuffer_params_default.restype = None
    L.rene_gbuffer_bytes.argtypes = [u32, u32]
    L.rene_gbuffer_bytes.restype = C.c_size_t
    L.rene_gbuffer.argtypes = [vp, C.POINTER(abi.GbufferParams), vp, C.c_size_t]
    L.rene_gbuffer_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rene_download_gbuffer.argtypes = [vp, vp, C.c_size_t]
    L.rene_primary_hits.argtypes = [vp, u32, u32, vp, C.c_size_t]
    L.rene_occlusion_params_default.argtypes = [C.POINTER(abi.OcclusionParams)]
    L.rene_occlusion_params_default.restype = None
    L.rene_occlusion_bytes.argtypes = [u32, u32]
    L.rene_occlusion_bytes.restype = C.c_size_t
    L.rene_occlusion.argtypes = [vp, C.POINTER(abi.OcclusionParams), vp, C.c_size_t]
    L.rene_occlusion_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rene_download_occlusion.argtypes = [vp, vp, C.c_size_t]
    L.rene_occlusion_samples.argtypes = [vp, C.POINTER(abi.OcclusionParams), vp, C.c_size_t]
    L.rene_direct_params_default.argtypes = [C.POINTER(abi.DirectParams)]
    L.rene_direct_params_default.restype = None
    L.rene_direct_bytes.argtypes = [u32, u32]
    L.rene_direct_bytes.restype = C.c_size_t
    L.rene_direct.argtypes = [vp, C.POINTER(abi.DirectParams), vp, C.c_size_t]
    L.rene_direct_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rene_download_direct.argtypes = [vp, vp, C.c_size_t]
    L.rene_direct_samples.argtypes = [vp, C.POINTER(abi.DirectParams), vp, C.c_size_t]
    L.rene_bounces_params_default.argtypes = [C.POINTER(abi.BouncesParams)]
    L.rene_bounces_params_default.restype = None
    L.rene_bounces_bytes.argtypes = [u32, u32]
    L.rene_bounces_bytes.restype = C.c_size_t
    L.rene_bounces.argtypes = [vp, C.POINTER(abi.BouncesParams), vp, C.c_size_t]
    L.rene_bounces_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rene_download_bounces.argtypes = [vp, vp, C.c_size_t]
    L.rene_bounces_samples.argtypes = [vp, C.POINTER(abi.BouncesParams), vp, C.c_size_t]
    L.rene_lights_params_default.argtypes = [C.POINTER(abi.LightsParams)]
    L.rene_lights_params_default.restype = None
    L.rene_lights_bytes.argtypes = [u32, u32]
    L.rene_lights_bytes.restype = C.c_size_t
    L.rene_lights_default_groups.argtypes = [vp, vp, u32, vp, u32, C.POINTER(C.c_uint8), C.POINTER(u32)]
    L.rene_lights.argtypes = [vp, C.POINTER(abi.LightsParams), vp, C.c_size_t]
    L.rene_lights_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rene_download_lights.argtypes = [vp, vp, C.c_size_t]
    L.rene_lights_samples.argtypes = [vp, C.POINTER(abi.LightsParams), vp, C.c_size_t]
    L.rene_exr_params_default.argtypes = [C.POINTER(abi.ExrParams)]
    L.rene_exr_params_default.restype = None
    L.rene_exr_layout.argtypes = [u32, u32, u32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(u32)]
    L.rene_exr_header.argtypes = [u32, u32, u32, vp, C.c_size_t]
    L.rene_output_exr.argtypes = [vp, C.POINTER(abi.ExrParams), vp, C.c_size_t]
    L.rene_exr_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rene_download_exr.argtypes = [vp, vp, C.c_size_t]
    L.rene_write_exr.argtypes = [vp, C.POINTER(abi.ExrParams), C.c_char_p]
    L.rene_exr_body_host.argtypes = [u32, u32, u32, C.POINTER(abi.ExrPlanes), vp, C.c_size_t]
    L.rene_exr_tail_bound.argtypes = [u32, u32, u32]
    L.rene_exr_tail_bound.restype = C.c_size_t
    L.rene_exr_attributes.argtypes = [u32, u32, u32, u32, vp, C.c_size_t]
    L.rene_exr_compress_host.argtypes = [u32, u32, u32, u32, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rene_exr_compress.argtypes = [vp, u32, u32, u32, u32, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rene_exr_tail_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rene_download_exr_tail.argtypes = [vp, vp, C.c_size_t]
    L.rene_output_exr_compressed.argtypes = [vp, C.POINTER(abi.ExrParams), u32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rene_write_exr_compressed.argtypes = [vp, C.POINTER(abi.ExrParams), u32, C.c_char_p]
    L.rene_exr_compress_rows_host.argtypes = [u32, u32, C.c_size_t, u32, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rene_exr_compress_rows.argtypes = [vp, u32, u32, C.c_size_t, u32, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    layers = C.POINTER(abi.CryptomatteLayer)
    L.rene_cryptomatte_params_default.argtypes = [C.POINTER(abi.CryptomatteParams)]
    L.rene_cryptomatte_params_default.restype = None
    L.rene_cryptomatte_hash.argtypes = [C.c_char_p, C.c_size_t]
    L.rene_cryptomatte_hash.restype = u32
    L.rene_cryptomatte_manifest.argtypes = [C.POINTER(C.c_char_p), u32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rene_cryptomatte_layout.argtypes = [u32, u32, layers, u32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(u32)]
    L.rene_cryptomatte_attributes.argtypes = [u32, u32, layers, u32, u32, vp, C.c_size_t]
    L.rene_cryptomatte_body_host.argtypes = [u32, u32, layers, u32, C.POINTER(vp), vp, C.c_size_t]
    L.rene_output_cryptomatte.argtypes = [vp, C.POINTER(abi.CryptomatteParams), vp, C.c_size_t]
    L.rene_cryptomatte_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rene_download_cryptomatte.argtypes = [vp, vp, C.c_size_t]
    L.rene_write_cryptomatte.argtypes = [vp, C.POINTER(abi.CryptomatteParams), u32, C.c_char_p]
    passes = C.POINTER(abi.ExrPassesParams)
    L.rene_exr_passes_params_default.argtypes = [passes]
    L.rene_exr_passes_params_default.restype = None
    L.rene_exr_passes_layout.argtypes = [u32, u32, passes, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(u32)]
    L.rene_exr_passes_attributes.argtypes = [u32, u32, passes, u32, vp, C.c_size_t]
    L.rene_exr_passes_body_host.argtypes = [u32, u32, passes, vp, vp, C.c_size_t]
    L.rene_output_exr_passes.argtypes = [vp, passes, vp, C.c_size_t]
    L.rene_exr_passes_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rene_download_exr_passes.argtypes = [vp, vp, C.c_size_t]
    L.rene_write_exr_passes.argtypes = [vp, passes, u32, C.c_char_p]
    L.rene_state_params_default.argtypes = [C.POINTER(abi.StateParams)]
    L.rene_state_params_default.restype = None
    L.rene_scene_fingerprint.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(C.c_uint64)]
    L.rene_state_bytes.argtypes = [u32, u32, u32, u32]
    L.rene_state_bytes.restype = C.c_size_t
    L.rene_save_state.argtypes = [vp, C.POINTER(abi.StateParams), vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rene_restore_state.argtypes = [vp, C.POINTER(abi.StateParams), C.POINTER(vp), C.POINTER(C.c_size_t), C.c_size_t]
    L.rene_state_inspect.argtypes = [vp, C.c_size_t, C.POINTER(abi.StateInfo)]
    L.rene_state_tiles.argtypes = [vp, C.c_size_t, vp, C.c_size_t]
    L.rene_state_verify.argtypes = [vp, C.c_size_t]
    L.rene_state_inspect_file.argtypes = [C.c_char_p, C.POINTER(abi.StateInfo), vp, C.c_size_t]
    L.rene_save_state_file.argtypes = [vp, C.POINTER(abi.StateParams), C.c_char_p]
    L.rene_restore_state_files.argtypes = [vp, C.POINTER(abi.StateParams), C.POINTER(C.c_char_p), C.c_size_t]
    L.rene_trace.argtypes = [vp, i32, C.c_size_t, vp, vp, C.c_float, C.c_float, vp]
    L.rene_bsdf_eval.argtypes = [vp, u32, C.c_size_t, vp, vp, vp, vp, vp, vp]
    L.rene_medium_eval.argtypes = [vp, u32, C.c_size_t, vp, vp, vp, vp, vp, vp]
    L.rene_transmittance.argtypes = [vp, C.c_int, u32, C.c_size_t, vp, vp, vp]
    L.rene_emitter_pdf.argtypes = [vp, C.c_size_t, vp, vp, vp]
    L.rene_emitter_pdf_form.argtypes = [vp, C.c_int, C.c_size_t, vp, vp, vp]
    L.rene_emit_sample.argtypes = [vp, C.c_int, C.c_size_t, vp, vp]
    L.rene_pcg_probe.argtypes = [i32, u32, u32, vp]
    L.rene_frame_stream_probe.argtypes = [vp, u32, u32, vp]
    L.rene_load_chains.argtypes = [vp, vp, C.c_size_t, u32, u32, vp, C.c_size_t]
    L.rene_ray_dump.argtypes = [vp, u32, u32, C.c_size_t, vp, C.POINTER(C.c_uint64)]
    L.rene_trace_queue.argtypes = [vp, C.c_size_t, vp, vp, i32, u32, u32, u32, u32, vp, C.POINTER(C.c_float), vp]
    L.rene_comm_unique_id.argtypes = [vp]
    L.rene_comm_init.argtypes = [vp, i32, i32, vp]
    L.rene_comm_init_all.argtypes = [C.POINTER(vp), i32]
    L.rene_reduce.argtypes = [vp, i32]
    L.rene_gather_tiles.argtypes = [vp, i32]
    L.rene_destroy.argtypes = [vp]
    L.rene_scene_pack_info.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.PackInfo)]
    L.rene_scene_small_items.argtypes = [C.POINTER(abi.SceneDesc), C.c_int, vp, u32, C.POINTER(u32), C.POINTER(u32)]
    L.rene_plan_memory.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.Opts), C.POINTER(abi.MemoryPlan)]
    L.rene_destroy.restype = None
    L.rene_last_error.restype = C.c_char_p
    L.rene_abi_version.restype = u32
    L.rene_to_rgb8.argtypes = [vp, C.c_size_t, u32, vp]
    L.rene_to_rgb8.restype = None
    L.rene_to_aov8.argtypes = [vp, C.c_size_t, u32, i32, vp]
    L.rene_to_aov8.restype = None
    L.rene_frame_seeds.argtypes = [u32, u32, u32, vp]
    L.rene_frame_seeds.restype = None
    L.rene_scene_load_pbrt.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.rene_scene_parse_pbrt.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(vp)]
    L.rene_scene_get_desc.argtypes = [vp]
    L.rene_scene_get_desc.restype = C.POINTER(abi.SceneDesc)
    L.rene_scene_film_filename.argtypes = [vp]
    L.rene_scene_film_filename.restype = C.c_char_p
    L.rene_scene_instance_name.argtypes = [vp, u32]
    L.rene_scene_instance_name.restype = C.c_char_p
    L.rene_scene_material_name.argtypes = [vp, u32]
    L.rene_scene_material_name.restype = C.c_char_p
    L.rene_scene_free.argtypes = [vp]
    L.rene_scene_free.restype = None
    if L.rene_abi_version() != abi.ABI_VERSION:
        raise ReneError(-1, "librene_hip.so ABI version differs from rene_amd.abi")
    _LIB = L
    return L


def _check(rc: int):
    if rc != 0:
        raise ReneError(rc, lib().rene_last_error().decode(errors="replace"))


# What the passes that leave a result in a device buffer of the library's own share (features, rgb8, gbuffer, the denoiser's buffers)
def _result_buffer(self, getter) -> tuple[int, int]:
    """(device pointer, bytes) of the result one of the library's rene_*_buffer calls hands out."""
    ptr, n = C.c_void_p(), C.c_size_t()
    _check(getter(self._h, C.byref(ptr), C.byref(n)))
    return ptr.value, n.value


def _download_result(self, download, shape, dtype) -> np.ndarray:
    """The result one of the library's rene_download_* calls copies out, as a fresh array."""
    out = np.empty(shape, dtype)
    _check(download(self._h, out.ctypes.data_as(C.c_void_p), out.nbytes))
    return out


def _check_tensor(name, tensor, device, dtypes, shape=None, numel=None, what="image") -> str:
    """A caller's torch tensor as the destination of `name`(): one of `dtypes` (returned), of `shape` (that of the `what`) or of `numel` bytes,
    contiguous, on GPU `device`; and torch's work on it has finished."""
    import torch  # (lazily: nothing else here needs it)
    if not isinstance(tensor, torch.Tensor):
        raise TypeError(f"{name}() takes a torch.Tensor")
    dtype = str(tensor.dtype).removeprefix("torch.")
    if dtype not in dtypes:
        raise TypeError(f"{name}(): the tensor must be {' or '.join(dtypes)}, not {tensor.dtype}")
    if shape is not None and tuple(tensor.shape) != shape:
        raise ValueError(f"{name}(): the tensor's shape is {tuple(tensor.shape)}, the {what}'s {shape}")
    if numel is not None and tensor.numel() != numel:
        raise ValueError(f"{name}(): the tensor has {tensor.numel()} bytes, the records {numel}")
    if not tensor.is_contiguous():
        raise ValueError(f"{name}(): the tensor must be contiguous")
    if tensor.device.type != "cuda" or (tensor.device.index or 0) != device:
        raise ValueError(f"{name}(): the tensor is on {tensor.device}, the context on GPU {device}")
    torch.cuda.current_stream(tensor.device).synchronize()  # work of torch's on the tensor (its fill, say) is not ordered with the context's stream
    return dtype


HIT_DTYPE = np.dtype([("t", np.float32), ("u", np.float32), ("v", np.float32),
                      ("instance", np.uint32), ("primitive", np.uint32)])


class Renderer:
    """One render context on one GPU: upload once, render frame ranges, read the 3 layers back
    (rene/src/main.rs:513, 1315-1397, 1453-1623)."""

    def __init__(self, scene, seed: int = abi.DEFAULT_SEED, device: int = 0, flags: int = 0,
                 shard_mode: int = abi.SHARD_TILES, shard_rank: int = 0, shard_count: int = 1,
                 framebuffer_ptr: int | None = None, stream_ptr: int | None = None):
        self._h = C.c_void_p()
        packed = scene if hasattr(scene, "byref") else scene.to_desc()
        self._packed = packed
        self._scene = scene  # (cryptomatte() asks it for the names of its instances and materials)
        o = abi.Opts()
        o.struct_size = C.sizeof(abi.Opts)
        o.seed, o.device, o.flags = seed & 0xFFFFFFFF, device, flags
        self._flags = flags
        self._shard_mode, self._shard_rank, self._shard_count = shard_mode, shard_rank, shard_count
        self.device = device
        o.shard_mode, o.shard_rank, o.shard_count = shard_mode, shard_rank, shard_count
        o.framebuffer = framebuffer_ptr
        o.stream = stream_ptr
        _check(lib().rene_create(packed.byref(), C.byref(o), C.byref(self._h)))
        self.xres, self.yres = packed.xres, packed.yres

    def close(self):
        if getattr(self, "_h", None):
            lib().rene_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render(self, first_frame: int, n_frames: int):
        _check(lib().rene_render(self._h, first_frame, n_frames))

    def sync(self):
        _check(lib().rene_sync(self._h))

    def reset(self):
        _check(lib().rene_reset(self._h))

    def tune(self, n_frames: int):
        """rene_tune: pick the work-item granularity for launches of n_frames frames; resets the image."""
        _check(lib().rene_tune(self._h, n_frames))

    def download(self, layer: int = abi.LAYER_RADIANCE, channels: int = 3) -> np.ndarray:
        out = np.empty((self.yres, self.xres, channels), dtype=np.float32)
        _check(lib().rene_download(self._h, layer, channels, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def stats(self) -> abi.Stats:
        st = abi.Stats()
        _check(lib().rene_get_stats(self._h, C.byref(st)))
        return st

    def framebuffer(self) -> tuple[int, int]:
        p, n = C.c_void_p(), C.c_size_t()
        _check(lib().rene_framebuffer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def trace(self, origins, directions, tmin: float = 0.001, tmax: float = 1e5, which: int = 0) -> np.ndarray:
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("origins and directions differ in shape")
        out = np.zeros(o.shape[0], dtype=HIT_DTYPE)
        _check(lib().rene_trace(self._h, which, o.shape[0], o.ctypes.data_as(C.c_void_p),
                                d.ctypes.data_as(C.c_void_p), tmin, tmax, out.ctypes.data_as(C.c_void_p)))
        return out


def denoise_params_default() -> abi.DenoiseParams:
    """rene_denoise_params_default: the `atrous` denoiser's constants (host only)."""
    p = abi.DenoiseParams()
    lib().rene_denoise_params_default(C.byref(p))
    return p


def _denoise_params(name, params) -> abi.DenoiseParams:
    p = denoise_params_default()
    for k, v in params.items():
        if k not in dict(abi.DenoiseParams._fields_) or k in ("struct_size", "reserved"):
            raise TypeError(f"{name}() got an unexpected parameter {k!r}")
        setattr(p, k, v)
    return p


def denoise_robust_params_default() -> abi.RobustParams:
    """rene_denoise_robust_params_default: the trimmed prepare's constants -- the robust resolve's with a gain of 0.35 (host only)."""
    p = abi.RobustParams()
    lib().rene_denoise_robust_params_default(C.byref(p))
    return p


def _denoise_call(self, name, plain, trimmed, robust, params):
    p = _denoise_params(name, params)
    if robust is None or robust is False:
        _check(plain(self._h, C.byref(p)))
        return
    if robust is True:
        robust = denoise_robust_params_default()
    if not isinstance(robust, abi.RobustParams):
        raise TypeError(f"{name}(robust=...) takes True or a RobustParams, not {type(robust).__name__}")
    _check(trimmed(self._h, C.byref(p), C.byref(robust)))


def _denoise(self, robust=None, **params):
    """rene_denoise: filter the frames accumulated so far on the device (include/rene_hip.h states the filter).  Keyword arguments replace
    fields of the defaults: iterations, sigma_luminance, sigma_normal2, sigma_albedo2, albedo_floor, relative_floor.
    robust = True or a RobustParams (denoise_robust_params_default(): max_trim 3, gain 0.35): rene_denoise_robust, the same filter prepared from
    the chains that do not stand out -- for scenes whose noise is fireflies; download_denoised(DENOISED_TRIM) says what was left out."""
    _denoise_call(self, "denoise", lib().rene_denoise, lib().rene_denoise_robust, robust, params)


def _denoise_tiles(self, robust=None, **params):
    """rene_denoise_tiles: the same filter tile by tile, for a context whose tiles differ in their frame counts (set_active_tiles): every tile
    with the constants of its own count, tiles with frames in fewer than two chains left unfiltered.  The same keyword arguments (robust = ...:
    rene_denoise_tiles_robust); the result through download_denoised (what = DENOISED_MEAN: the filtered mean image) and denoised_buffer."""
    _denoise_call(self, "denoise_tiles", lib().rene_denoise_tiles, lib().rene_denoise_tiles_robust, robust, params)


def _download_denoised(self, what: int = abi.DENOISED_RADIANCE, channels: int = 3) -> np.ndarray:
    """The last denoise()'s or denoise_tiles()'s radiance sums (what = DENOISED_RADIANCE, channels 3 or 4: divide by the frame count -- the tile's,
    after denoise_tiles -- or hand to to_rgb8), its filtered mean image (what = DENOISED_MEAN, channels 3 or 4), its unfiltered variance plane
    (what = DENOISED_VARIANCE; an (yres, xres) array) or the chains it trimmed from either end of every pixel (what = DENOISED_TRIM; an (yres, xres)
    array, zeros unless the call was made with robust = ...)."""
    plane = what in (abi.DENOISED_VARIANCE, abi.DENOISED_TRIM)
    if plane:
        channels = 1
    out = np.empty((self.yres, self.xres, channels), dtype=np.float32)
    _check(lib().rene_download_denoised(self._h, what, channels, out.ctypes.data_as(C.c_void_p), out.size))
    return out[..., 0] if plane else out


def _denoised_buffer(self) -> tuple[int, int]:
    return _result_buffer(self, lib().rene_denoised_buffer)


def denoise_shard_bytes(xres: int, yres: int, shard_rank: int = 0, shard_count: int = 1) -> int:
    """rene_denoise_shard_bytes: the size of the packed buffer denoise_shard_prepare() makes on tile shard `shard_rank` of `shard_count` of an
    xres x yres film -- header, per-tile table, 52 bytes per owned pixel slot (host only; 0 for arguments that describe no shard)."""
    return int(lib().rene_denoise_shard_bytes(xres, yres, shard_rank, shard_count))


def _denoise_shard_prepare(self, **params):
    """rene_denoise_shard_prepare: the denoiser's per-pixel half on the tiles this context owns (a tile shard, or an unsharded context as a shard
    of one), into the context's packed buffer.  The keyword arguments of denoise().  Call it before gather_tiles() / reduce(), which consume the
    frame chains; the buffer stays usable afterwards."""
    p = _denoise_params("denoise_shard_prepare", params)
    _check(lib().rene_denoise_shard_prepare(self._h, C.byref(p)))


def _denoise_shard_buffer(self) -> tuple[int, int]:
    """rene_denoise_shard_buffer: (device pointer, bytes) of the last denoise_shard_prepare()'s packed buffer."""
    return _result_buffer(self, lib().rene_denoise_shard_buffer)


def _download_denoise_shard(self) -> np.ndarray:
    """rene_download_denoise_shard: the packed buffer as a uint8 array (include/rene_hip.h has its layout)."""
    return _download_result(self, lib().rene_download_denoise_shard, _denoise_shard_buffer(self)[1], np.uint8)


def _denoise_place_shard(self, src, n_bytes: int | None = None):
    """rene_denoise_place_shard on this context, the root: `src` is a shard's packed buffer, either a (device pointer, bytes) pair as
    denoise_shard_buffer() returns it (or the pointer and n_bytes), or a host array as download_denoise_shard() returns it."""
    if isinstance(src, tuple):
        src, n_bytes = src
    if isinstance(src, (int, np.integer)):
        if n_bytes is None:
            raise TypeError("denoise_place_shard(): a device pointer needs its size in bytes")
        _check(lib().rene_denoise_place_shard(self._h, C.c_void_p(int(src)), int(n_bytes)))
        return
    a = np.ascontiguousarray(src)
    _check(lib().rene_denoise_place_shard(self._h, a.ctypes.data_as(C.c_void_p), a.nbytes if n_bytes is None else n_bytes))


def _denoise_placed(self):
    """rene_denoise_placed: filter the records placed on this context -- every rank of the shard layout must have been placed since the last
    completed filter.  The result through download_denoised() and denoised_buffer(), as after denoise_tiles()."""
    _check(lib().rene_denoise_placed(self._h))


def _gather_denoise(self, root: int = 0):
    """rene_gather_denoise: the packed buffers' way over the communicator (comm_init), every rank after its denoise_shard_prepare(); the root
    places what it received at the start of its denoise_placed()."""
    _check(lib().rene_gather_denoise(self._h, root))


def denoise_shards(renderers, root: int = 0, via: str = "device", **params):
    """Denoise a job whose tile shards live in this process: prepare on every shard, place every packed buffer on renderers[root] -- from its
    device pointer (via = "device") or through host memory (via = "host") -- and filter there.  `renderers` in rank order, all of them; the keyword
    arguments of denoise().  Returns renderers[root], whose download_denoised() / denoised_buffer() hand out the result."""
    if via not in ("device", "host"):
        raise ValueError('denoise_shards(): via must be "device" or "host"')
    renderers = list(renderers)
    for r in renderers:
        r.denoise_shard_prepare(**params)
    for r in renderers:
        renderers[root].denoise_place_shard(r.denoise_shard_buffer() if via == "device" else r.download_denoise_shard())
    renderers[root].denoise_placed()
    return renderers[root]


Renderer.denoise_shard_prepare = _denoise_shard_prepare
Renderer.denoise_shard_buffer = _denoise_shard_buffer
Renderer.download_denoise_shard = _download_denoise_shard
Renderer.denoise_place_shard = _denoise_place_shard
Renderer.denoise_placed = _denoise_placed
Renderer.gather_denoise = _gather_denoise
Renderer.denoise = _denoise
Renderer.denoise_tiles = _denoise_tiles
Renderer.download_denoised = _download_denoised
Renderer.denoised_buffer = _denoised_buffer


def noise_params_default() -> abi.NoiseParams:
    """rene_noise_params_default: the noise estimate's constant (host only)."""
    p = abi.NoiseParams()
    lib().rene_noise_params_default(C.byref(p))
    return p


def noise_combine(parts) -> abi.NoiseEstimate:
    """rene_noise_combine: the estimate of a tile-sharded job from its shards' estimates (host only)."""
    parts = list(parts)
    arr = (abi.NoiseEstimate * max(1, len(parts)))(*parts)
    out = abi.NoiseEstimate()
    _check(lib().rene_noise_combine(arr, len(parts), C.byref(out)))
    return out


def noise_frames_needed(estimate: abi.NoiseEstimate, target: float) -> int:
    """rene_noise_frames_needed: the frames a job needs for `target` by the 1 / sqrt(N) law -- ceil(N (noise / target)^2), at least N, saturating."""
    return int(lib().rene_noise_frames_needed(C.byref(estimate), float(target)))


def _estimate_noise(self, **params) -> abi.NoiseEstimate:
    """rene_estimate_noise: the noise of the frames accumulated so far, for the image and per 32 x 32 tile (include/rene_hip.h states the metric).
    Keyword arguments replace fields of the defaults: luminance_floor."""
    p = noise_params_default()
    for k, v in params.items():
        if k != "luminance_floor":
            raise TypeError(f"estimate_noise() got an unexpected parameter {k!r}")
        setattr(p, k, v)
    out = abi.NoiseEstimate()
    _check(lib().rene_estimate_noise(self._h, C.byref(p), C.byref(out)))
    return out


def _noise_tiles(self) -> np.ndarray:
    """The last estimate_noise()'s tile records on the full grid: a (tiles_y, tiles_x) structured array with fields sum_var, sum_lum, n_pixels
    (tiles this context does not own are zero)."""
    ty, tx = (self.yres + abi.TILE_SIZE - 1) // abi.TILE_SIZE, (self.xres + abi.TILE_SIZE - 1) // abi.TILE_SIZE
    out = np.zeros((ty, tx), dtype=np.dtype(abi.NOISE_TILE_DTYPE))
    _check(lib().rene_download_noise_tiles(self._h, out.ctypes.data_as(C.c_void_p), out.size))
    return out


def next_batch(done: int, needed: int, batch: int, max_frames: int) -> int:
    """The schedule of render_until and of `rene-hip --target-noise`: half of what the estimate says is missing (one render's prediction
    scatters between 0.75 and 1.35 times the truth), at least `batch`, rounded up to a multiple of 8, capped by what is left of max_frames."""
    n = max(batch, (max(needed, done) - done + 1) // 2)
    n = (n + 7) // 8 * 8
    return min(n, max_frames - done)


def _render_until(self, target: float, max_frames: int, batch: int = 64, first_frame: int = 0):
    """Render frames first_frame, first_frame + 1, ... until estimate_noise().noise <= target or max_frames frames are done: (frames rendered,
    the last estimate).  The image is bit for bit that of one render(first_frame, frames).  `batch`, the first batch, is a multiple of 8 and at
    least 16, so that every chain holds two frames or more when the first estimate is taken."""
    if batch < 16 or batch % 8:
        raise ValueError("render_until: batch must be a multiple of 8 and at least 16")
    if not target > 0:
        raise ValueError("render_until: target must be positive")
    if max_frames < 2:
        raise ValueError("render_until: max_frames must be at least 2")
    done = min(batch, max_frames)
    self.render(first_frame, done)
    est = self.estimate_noise()
    while est.noise > target and done < max_frames:
        n = next_batch(done, noise_frames_needed(est, target), batch, max_frames)
        self.render(first_frame + done, n)
        done += n
        est = self.estimate_noise()
    return done, est


Renderer.estimate_noise = _estimate_noise
Renderer.noise_tiles = _noise_tiles
Renderer.render_until = _render_until


# ---- adaptive sampling (include/rene_hip.h: rene_set_active_tiles and what follows it) ----------------------------------------------------------
def _tile_grid(self) -> tuple[int, int]:
    return (self.yres + abi.TILE_SIZE - 1) // abi.TILE_SIZE, (self.xres + abi.TILE_SIZE - 1) // abi.TILE_SIZE


def _set_active_tiles(self, active):
    """rene_set_active_tiles: `active` is a (tiles_y, tiles_x) array, non-zero = the tile goes on rendering (None: all).  The set only shrinks until
    reset(); entries of tiles this context does not own are ignored."""
    if active is None:
        _check(lib().rene_set_active_tiles(self._h, None, 0))
        return
    a = np.ascontiguousarray(np.asarray(active) != 0, dtype=np.uint8)
    if a.shape != _tile_grid(self):
        raise ValueError(f"set_active_tiles: expected a {_tile_grid(self)} array, got {a.shape}")
    _check(lib().rene_set_active_tiles(self._h, a.ctypes.data_as(C.c_void_p), a.size))


def _tile_frames(self) -> np.ndarray:
    """rene_tile_frames: the frames every tile has received, (tiles_y, tiles_x) uint32 (tiles this context does not own are zero)."""
    out = np.zeros(_tile_grid(self), np.uint32)
    _check(lib().rene_tile_frames(self._h, out.ctypes.data_as(C.c_void_p), out.size))
    return out


def _download_mean(self, layer: int = abi.LAYER_RADIANCE, channels: int = 3) -> np.ndarray:
    """rene_download_mean: download() with every pixel divided by its tile's frame count on the device (tiles without frames are zero)."""
    out = np.empty((self.yres, self.xres, channels), dtype=np.float32)
    _check(lib().rene_download_mean(self._h, layer, channels, out.ctypes.data_as(C.c_void_p), out.size))
    return out


def noise_select_tiles(tiles, active_in, target: float, dilate: int = 1, luminance_floor: float = 0.01) -> np.ndarray:
    """rene_noise_select_tiles (host only): which tiles of an adaptive job go on -- those active in `active_in` (None: all) that have pixels and
    lie within `dilate` steps (Chebyshev) of an active tile whose noise sqrt(q_t) exceeds `target`.  `tiles`: noise_tiles()'s (tiles_y, tiles_x)
    records.  A (tiles_y, tiles_x) uint8 array."""
    t = np.ascontiguousarray(tiles, dtype=np.dtype(abi.NOISE_TILE_DTYPE))
    if t.ndim != 2:
        raise ValueError("noise_select_tiles: tiles must be a (tiles_y, tiles_x) array of tile records")
    a = None if active_in is None else np.ascontiguousarray(np.asarray(active_in) != 0, dtype=np.uint8)
    if a is not None and a.shape != t.shape:
        raise ValueError("noise_select_tiles: active_in and tiles differ in shape")
    out = np.zeros(t.shape, np.uint8)
    _check(lib().rene_noise_select_tiles(t.ctypes.data_as(C.c_void_p), None if a is None else a.ctypes.data_as(C.c_void_p), t.shape[1], t.shape[0],
                                         luminance_floor, float(target), dilate, out.ctypes.data_as(C.c_void_p)))
    return out


def tile_noise(tiles, luminance_floor: float = 0.01) -> np.ndarray:
    """q_t of noise_tiles()'s records as the library takes it (fp64; 0 where a tile has no pixels or was not estimated): the tile noise is its root."""
    n = tiles["n_pixels"].astype(np.float64)
    ok = n > 0
    q = np.zeros(tiles.shape, np.float64)
    m = tiles["sum_lum"][ok].astype(np.float64) / n[ok] + float(np.float32(luminance_floor))
    q[ok] = (tiles["sum_var"][ok].astype(np.float64) / n[ok]) / (m * m)
    return q


def _render_adaptive(self, target: float, max_frames: int, batch: int = 64, dilate: int = 1, first_frame: int = 0):
    """Render until every TILE's noise sqrt(q_t) is at most `target` or max_frames frames are done, switching off the tiles that have met it:
    (tile_frames(), the last estimate).  After the first batch and after every further one the noise is estimated and noise_select_tiles picks
    the tiles that go on; the quietest of them sets the next batch -- next_batch(done, min over active tiles of ceil(done q_t / target^2), ...) --
    so no tile overshoots by more than the schedule's half-step.  Every tile's image is bit for bit that of render(first_frame, N_t); the sums
    handed out by download() are over N_t frames per tile: use download_mean().  The context must be fresh (or reset): first_frame is where
    its frames begin."""
    if batch < 16 or batch % 8:
        raise ValueError("render_adaptive: batch must be a multiple of 8 and at least 16")
    if not target > 0:
        raise ValueError("render_adaptive: target must be positive")
    if max_frames < 2:
        raise ValueError("render_adaptive: max_frames must be at least 2")
    done = min(batch, max_frames)
    self.render(first_frame, done)
    est = self.estimate_noise()
    floor = est.luminance_floor
    active = None
    while True:
        tiles = self.noise_tiles()
        active = noise_select_tiles(tiles, active, target, dilate, floor)
        if not active.any() or done >= max_frames:
            break
        self.set_active_tiles(active)
        q = tile_noise(tiles, floor)[active != 0]
        needed = int(min(np.ceil(done * q / (target * target)).min(), 0xFFFFFFFF))
        n = next_batch(done, needed, batch, max_frames)
        self.render(first_frame + done, n)
        done += n
        est = self.estimate_noise()
    return self.tile_frames(), est


Renderer.set_active_tiles = _set_active_tiles
Renderer.tile_frames = _tile_frames
Renderer.download_mean = _download_mean
Renderer.render_adaptive = _render_adaptive


# ---- the firefly-robust resolve (include/rene_hip.h: rene_resolve_robust) -----------------------------------------------------------------------
def robust_params_default() -> abi.RobustParams:
    """rene_robust_params_default: the robust resolve's constants (host only)."""
    p = abi.RobustParams()
    lib().rene_robust_params_default(C.byref(p))
    return p


def robust_combine(parts) -> abi.RobustSummary:
    """rene_robust_combine: the summary of a tile-sharded job from its shards' summaries (host only)."""
    parts = list(parts)
    arr = (abi.RobustSummary * max(1, len(parts)))(*parts)
    out = abi.RobustSummary()
    _check(lib().rene_robust_combine(arr, len(parts), C.byref(out)))
    return out


def _resolve_robust(self, **params) -> abi.RobustSummary:
    """rene_resolve_robust: the trimmed mean of the frames accumulated so far over the eight frame chains (include/rene_hip.h states the rule).
    Keyword arguments replace fields of the defaults: max_trim, gain.  The image: download_robust()."""
    p = robust_params_default()
    for k, v in params.items():
        if k not in ("max_trim", "gain"):
            raise TypeError(f"resolve_robust() got an unexpected parameter {k!r}")
        setattr(p, k, v)
    out = abi.RobustSummary()
    _check(lib().rene_resolve_robust(self._h, C.byref(p), C.byref(out)))
    return out


def _download_robust(self, what: int = abi.ROBUST_IMAGE, channels: int = 3) -> np.ndarray:
    """The last resolve_robust()'s MEAN radiance (what = ROBUST_IMAGE, channels 3 or 4) or the chains it trimmed from either end of every pixel
    (what = ROBUST_TRIM; an (yres, xres) array of 0 .. 3).  Tiles this context does not own are zero."""
    if what == abi.ROBUST_TRIM:
        channels = 1
    out = np.empty((self.yres, self.xres, channels), dtype=np.float32)
    _check(lib().rene_download_robust(self._h, what, channels, out.ctypes.data_as(C.c_void_p), out.size))
    return out[..., 0] if what == abi.ROBUST_TRIM else out


def _robust_tiles(self) -> np.ndarray:
    """The last resolve_robust()'s tile records on the full grid: a (tiles_y, tiles_x) structured array with fields sum_lum_plain, sum_lum_robust,
    n_pixels, n_trimmed (tiles this context does not own are zero)."""
    out = np.zeros(_tile_grid(self), dtype=np.dtype(abi.ROBUST_TILE_DTYPE))
    _check(lib().rene_download_robust_tiles(self._h, out.ctypes.data_as(C.c_void_p), out.size))
    return out


Renderer.resolve_robust = _resolve_robust
Renderer.download_robust = _download_robust
Renderer.robust_tiles = _robust_tiles


# ---- the denoiser hand-off (include/rene_hip.h: rene_export_features) ---------------------------------------------------------------------------
def feature_params_default() -> abi.FeatureParams:
    """rene_feature_params_default: COLOR | ALBEDO | NORMAL, fp32, [H][W][C] (host only)."""
    p = abi.FeatureParams()
    lib().rene_feature_params_default(C.byref(p))
    return p


def feature_channels(features: int) -> int:
    """rene_feature_channels: the channels a feature mask selects, 0 for an empty mask or unknown bits (host only)."""
    return int(lib().rene_feature_channels(features & 0xffffffff))


_FEATURE_FORMATS = {"f32": (abi.FEATURES_F32, np.float32), "f16": (abi.FEATURES_F16, np.float16)}
_FEATURE_LAYOUTS = {"hwc": abi.FEATURES_HWC, "chw": abi.FEATURES_CHW}


def _feature_params(features, dtype, layout) -> abi.FeatureParams:
    if dtype not in _FEATURE_FORMATS:
        raise ValueError(f"dtype must be 'f32' or 'f16', not {dtype!r}")
    if layout not in _FEATURE_LAYOUTS:
        raise ValueError(f"layout must be 'hwc' or 'chw', not {layout!r}")
    p = feature_params_default()
    p.features, p.format, p.layout = features, _FEATURE_FORMATS[dtype][0], _FEATURE_LAYOUTS[layout]
    return p


def _feature_shape(self, channels, layout):
    return (self.yres, self.xres, channels) if layout == "hwc" else (channels, self.yres, self.xres)


def _features(self, features: int = abi.FEATURE_DEFAULT, dtype: str = "f32", layout: str = "hwc") -> np.ndarray:
    """rene_export_features into the library's own device buffer, downloaded: the MEANS of the frames accumulated so far as one tensor, the
    channels of the mask (abi.FEATURE_*) in bit order -- (yres, xres, C) for layout "hwc", (C, yres, xres) for "chw", float32 or float16.
    Tiles the context does not own are 0."""
    p = _feature_params(features, dtype, layout)
    _check(lib().rene_export_features(self._h, C.byref(p), None, 0))
    return _download_result(self, lib().rene_download_features, _feature_shape(self, feature_channels(features), layout), _FEATURE_FORMATS[dtype][1])


def _features_buffer(self):
    """rene_features_buffer: (device pointer, bytes) of the last features() result."""
    return _result_buffer(self, lib().rene_features_buffer)


def _features_into(self, tensor, features: int = abi.FEATURE_DEFAULT, layout: str = "hwc"):
    """rene_export_features into a caller-owned torch tensor on the context's device: contiguous, float32 or float16 (the element format follows
    the tensor), of shape (yres, xres, C) for layout "hwc" or (C, yres, xres) for "chw".  Only the pixels of the tiles this context owns are
    written, so the tile shards of one device fill one tensor between them.  Returns the tensor."""
    shape = _feature_shape(self, feature_channels(features), layout)
    dtype = _check_tensor("features_into", tensor, self.device, ("float32", "float16"), shape=shape, what="export")
    p = _feature_params(features, {"float32": "f32", "float16": "f16"}[dtype], layout)
    _check(lib().rene_export_features(self._h, C.byref(p), C.c_void_p(tensor.data_ptr()), tensor.numel() * tensor.element_size()))
    return tensor


Renderer.features = _features
Renderer.features_buffer = _features_buffer
Renderer.features_into = _features_into


# ---- the output transform on the device (include/rene_hip.h: rene_output_8bit) ------------------------------------------------------------------
_OUTPUT_SOURCES = {"radiance": abi.OUTPUT_RADIANCE, "normal": abi.OUTPUT_NORMAL, "albedo": abi.OUTPUT_ALBEDO, "denoised": abi.OUTPUT_DENOISED,
                   "denoised_mean": abi.OUTPUT_DENOISED_MEAN, "robust": abi.OUTPUT_ROBUST}
_OUTPUT_TRANSFORMS = {"srgb": abi.OUTPUT_SRGB, "aov": abi.OUTPUT_AOV, "aov_normal": abi.OUTPUT_AOV_NORMAL}


def output_params_default() -> abi.OutputParams:
    """rene_output_params_default: RADIANCE, RGB8 (host only)."""
    p = abi.OutputParams()
    lib().rene_output_params_default(C.byref(p))
    return p


def _output_params(source, alpha) -> abi.OutputParams:
    if source not in _OUTPUT_SOURCES:
        raise ValueError(f"source must be one of {sorted(_OUTPUT_SOURCES)}, not {source!r}")
    p = output_params_default()
    p.source, p.format = _OUTPUT_SOURCES[source], abi.OUTPUT_RGBA8 if alpha else abi.OUTPUT_RGB8
    return p


def _rgb8(self, source: str = "radiance", alpha: bool = False, *, tonemap=None, exposure=None, white=None, key=None) -> np.ndarray:
    """rene_output_8bit into the library's own device buffer, downloaded: the 8-bit image of `source` -- "radiance" (sRGB), "normal", "albedo" (the
    AOV transforms), "denoised", "denoised_mean", "robust" (sRGB, after their calls) -- as a (yres, xres, 3) uint8 array, or (yres, xres, 4) with
    alpha 255.  The bytes are those of to_rgb8() / to_aov8() on what the matching download hands out; 3 or 4 bytes per pixel cross PCIe.  Tiles
    the context does not own are 0.
    Any of the keywords makes it rene_output_tonemapped (the sRGB sources only): tonemap "clamp" (the default), "reinhard" or "aces"; exposure in
    EV, rounded to eighth-stops, or "auto" (from this context's luminance_stats(source) and `key`, the target in eighth-stops of log2, -20 by
    default: about 0.18); white, the Reinhard white point (4).  The bytes are those of tonemap_rgb8() on the source's means.  The tile shards of
    one image take one exposure from their combined statistics: exposure=auto_exposure_e8(luminance_combine(parts)) / 8."""
    tm = _tonemap_params(self, source, alpha, tonemap, exposure, white, key)
    if tm is not None:
        _check(lib().rene_output_tonemapped(self._h, C.byref(tm), None, 0))
    else:
        _check(lib().rene_output_8bit(self._h, C.byref(_output_params(source, alpha)), None, 0))
    return _download_result(self, lib().rene_download_output, (self.yres, self.xres, 4 if alpha else 3), np.uint8)


def _rgb8_buffer(self):
    """rene_output_buffer: (device pointer, bytes) of the last rgb8() result."""
    return _result_buffer(self, lib().rene_output_buffer)


def _rgb8_into(self, tensor, source: str = "radiance", alpha: bool = False, *, tonemap=None, exposure=None, white=None, key=None):
    """rene_output_8bit into a caller-owned torch tensor on the context's device: contiguous, uint8, of shape (yres, xres, 3), or (yres, xres, 4)
    with alpha.  Only the pixels of the tiles this context owns are written, so the tile shards of one device fill one tensor between them.
    tonemap, exposure, white, key: as for rgb8().  Returns the tensor."""
    _output_params(source, alpha)  # (an unknown source is refused before the tensor is looked at)
    _check_tensor("rgb8_into", tensor, self.device, ("uint8",), shape=(self.yres, self.xres, 4 if alpha else 3))
    tm = _tonemap_params(self, source, alpha, tonemap, exposure, white, key)
    if tm is not None:
        _check(lib().rene_output_tonemapped(self._h, C.byref(tm), C.c_void_p(tensor.data_ptr()), tensor.numel()))
    else:
        _check(lib().rene_output_8bit(self._h, C.byref(_output_params(source, alpha)), C.c_void_p(tensor.data_ptr()), tensor.numel()))
    return tensor


Renderer.rgb8 = _rgb8
Renderer.rgb8_buffer = _rgb8_buffer
Renderer.rgb8_into = _rgb8_into


# ---- the per-pixel frame-range passes: the geometry, occlusion, direct-light, bounce and light-group passes ---------------------------------------
class _PixelPass:
    """What one per-pixel frame-range pass (rene_<name>) differs from its siblings in -- its name, its params type, its record dtype (abi's
    constant `dtype_name`), the dtypes its *_into tensor may have, the defaults in words -- and, built from that, the functions that are the
    same for all of them: <name>_params_default, <name>_bytes, Renderer.<name>_buffer and <name>_merge under their public names, and run, into
    and records for the pass's own functions below.  The library's entry points are found by the name: rene_<name>, rene_<name>_params_default,
    _bytes, _buffer and rene_download_<name>."""

    def __init__(self, name, params_type, dtype_name, into_dtypes, defaults):
        self.name, self.dtype_name, self.into_dtypes = name, dtype_name, into_dtypes
        self.dtype = np.dtype(getattr(abi, dtype_name))
        entry, records = self._entry, self.records

        def params_default():
            p = params_type()
            entry("rene_{}_params_default")(C.byref(p))
            return p

        def bytes_(xres: int, yres: int) -> int:
            return int(entry("rene_{}_bytes")(xres, yres))

        def buffer(self):  # (a Renderer's method)
            return _result_buffer(self, entry("rene_{}_buffer"))

        def merge(parts) -> np.ndarray:
            parts = [records(p) for p in parts]
            if not parts or any(p.shape != parts[0].shape for p in parts):
                raise ValueError(f"{name}_merge() takes one or more record arrays of one shape")
            out = np.zeros(parts[0].shape, parts[0].dtype)
            for p in parts:
                own = p["n"] != 0
                if (out["n"][own] != 0).any():
                    raise ValueError(f"{name}_merge(): two parts hold the same pixel")
                out[own] = p[own]
            return out

        for f, public, doc in ((params_default, f"{name}_params_default", f"rene_{name}_params_default: {defaults} (host only)."),
                               (bytes_, f"{name}_bytes", f"rene_{name}_bytes: {self.dtype.itemsize} bytes per pixel (host only)."),
                               (buffer, f"_{name}_buffer", f"rene_{name}_buffer: (device pointer, bytes) of the last {name}() result."),
                               (merge, f"{name}_merge", "The union of tile shards' record arrays: every pixel's record from the part whose n != 0 (all zero "
                                                        "where no part has it).")):
            f.__name__ = f.__qualname__ = public
            f.__doc__ = doc
        params_default.__annotations__["return"] = f"abi.{params_type.__name__}"
        self.params_default, self.bytes, self.buffer, self.merge = params_default, bytes_, buffer, merge

    def _entry(self, pattern):
        return getattr(lib(), pattern.format(self.name))

    def run(self, r, params) -> np.ndarray:
        """rene_<name> into the library's own device buffer, downloaded: a (yres, xres) array of the pass's records."""
        _check(self._entry("rene_{}")(r._h, C.byref(params), None, 0))
        return _download_result(r, self._entry("rene_download_{}"), (r.yres, r.xres), self.dtype)

    def into(self, r, tensor, params):
        """rene_<name> into a caller-owned torch tensor on the context's device, of the record array's bytes.  Returns the tensor."""
        item = 4 if str(getattr(tensor, "dtype", "")) == "torch.int32" else 1
        _check_tensor(f"{self.name}_into", tensor, r.device, self.into_dtypes, numel=self.bytes(r.xres, r.yres) // item)
        _check(self._entry("rene_{}")(r._h, C.byref(params), C.c_void_p(tensor.data_ptr()), tensor.numel() * item))
        return tensor

    def records(self, rec) -> np.ndarray:
        rec = np.asarray(rec)
        if rec.dtype != self.dtype:
            raise TypeError(f"expected an array of abi.{self.dtype_name} records")
        return rec


_GBUFFER = _PixelPass("gbuffer", abi.GbufferParams, "GBUFFER_DTYPE", ("uint8",), "frames 0 .. 15, instance ids")
_OCCLUSION = _PixelPass("occlusion", abi.OcclusionParams, "OCCLUSION_DTYPE", ("uint8", "int32"), "frames 0 .. 15, one ray per hitting sample, radius 1")
_DIRECT = _PixelPass("direct", abi.DirectParams, "DIRECT_DTYPE", ("uint8", "int32"), "frames 0 .. 15")
gbuffer_params_default, gbuffer_bytes, gbuffer_merge, _gbuffer_records = _GBUFFER.params_default, _GBUFFER.bytes, _GBUFFER.merge, _GBUFFER.records
occlusion_params_default, occlusion_bytes, occlusion_merge, _occlusion_records = _OCCLUSION.params_default, _OCCLUSION.bytes, _OCCLUSION.merge, _OCCLUSION.records
_BOUNCES = _PixelPass("bounces", abi.BouncesParams, "BOUNCES_DTYPE", ("uint8", "int32"), "frames 0 .. 15, max_depth 0 (rene's own 50)")
direct_params_default, direct_bytes, direct_merge, _direct_records = _DIRECT.params_default, _DIRECT.bytes, _DIRECT.merge, _DIRECT.records
bounces_params_default, bounces_bytes, bounces_merge, _bounces_records = _BOUNCES.params_default, _BOUNCES.bytes, _BOUNCES.merge, _BOUNCES.records
_LIGHTS = _PixelPass("lights", abi.LightsParams, "LIGHTS_DTYPE", ("uint8", "int32"), "frames 0 .. 15, no tables: the library's own grouping")
lights_params_default, lights_bytes, lights_merge, _lights_records = _LIGHTS.params_default, _LIGHTS.bytes, _LIGHTS.merge, _LIGHTS.records


# ---- the geometry pass (rene_gbuffer): first-hit depth, position, coverage and id mattes --------------------------------------------------------
_GBUFFER_IDS = {"instance": abi.GBUFFER_ID_INSTANCE, "material": abi.GBUFFER_ID_MATERIAL, "primitive": abi.GBUFFER_ID_PRIMITIVE}


def _gbuffer_params(first_frame, n_frames, ids) -> abi.GbufferParams:
    if ids not in _GBUFFER_IDS:
        raise ValueError(f"ids must be one of {sorted(_GBUFFER_IDS)}, not {ids!r}")
    p = gbuffer_params_default()
    p.first_frame, p.n_frames, p.id_source = first_frame, n_frames, _GBUFFER_IDS[ids]
    return p


def _gbuffer(self, first_frame: int = 0, n_frames: int = 16, ids: str = "instance") -> np.ndarray:
    """rene_gbuffer into the library's own device buffer, downloaded: a (yres, xres) structured array of abi.GBUFFER_DTYPE -- per pixel the first
    hits of the primary rays of frames first_frame .. first_frame + n_frames - 1: depth_sum, depth_min, hits, n, position_sum, other and four
    (id, count) slots of `ids` ("instance", "material" or "primitive"), ordered by count.  Nothing of the accumulated image is read or changed.
    Pixels of tiles the context does not own are the all-zero record (n == 0): gbuffer_merge() joins the tile shards' arrays."""
    return _GBUFFER.run(self, _gbuffer_params(first_frame, n_frames, ids))


def _gbuffer_into(self, tensor, first_frame: int = 0, n_frames: int = 16, ids: str = "instance"):
    """rene_gbuffer into a caller-owned torch tensor on the context's device: contiguous, uint8, yres * xres * 64 elements (any shape).  All of it
    is written: zeros, then the records of the tiles this context owns.  Returns the tensor."""
    return _GBUFFER.into(self, tensor, _gbuffer_params(first_frame, n_frames, ids))


def _primary_hits(self, first_frame: int, n_frames: int) -> np.ndarray:
    """rene_primary_hits (probe): every sample gbuffer() aggregates, a (n_frames, yres, xres) structured array of abi.PRIMARY_HIT_DTYPE -- the
    primary ray's direction d, and t (-1: a miss), u, v, instance, primitive of its closest hit as Renderer.trace reports them."""
    out = np.zeros((max(int(n_frames), 0), self.yres, self.xres), abi.PRIMARY_HIT_DTYPE)
    _check(lib().rene_primary_hits(self._h, first_frame, n_frames, out.ctypes.data_as(C.c_void_p), out.size))
    return out


Renderer.gbuffer = _gbuffer
Renderer.gbuffer_buffer = _GBUFFER.buffer
Renderer.gbuffer_into = _gbuffer_into
Renderer.primary_hits = _primary_hits


# ---- the occlusion pass (rene_occlusion): ambient occlusion and bent normals from the first hit -------------------------------------------------
def _occlusion_params(first_frame, n_frames, rays, radius) -> abi.OcclusionParams:
    p = occlusion_params_default()
    p.first_frame, p.n_frames, p.rays, p.radius = first_frame, n_frames, rays, radius
    return p


def _occlusion(self, first_frame: int = 0, n_frames: int = 16, rays: int = 1, radius: float = 1.0) -> np.ndarray:
    """rene_occlusion into the library's own device buffer, downloaded: a (yres, xres) structured array of abi.OCCLUSION_DTYPE -- per pixel, over the
    first hits of the primary rays of frames first_frame .. first_frame + n_frames - 1 and `rays` cosine-distributed rays of length `radius` from
    each: hits, rays, occluded, n and bent_sum, the sum of the unoccluded directions.  occlusion_ao() and occlusion_bent() turn the records into
    images.  Nothing of the accumulated image is read or changed.  Pixels of tiles the context does not own are the all-zero record (n == 0):
    occlusion_merge() joins the tile shards' arrays."""
    return _OCCLUSION.run(self, _occlusion_params(first_frame, n_frames, rays, radius))


def _occlusion_into(self, tensor, first_frame: int = 0, n_frames: int = 16, rays: int = 1, radius: float = 1.0):
    """rene_occlusion into a caller-owned torch tensor on the context's device: contiguous, uint8 or int32, yres * xres * 32 bytes (any shape).  All
    of it is written: zeros, then the records of the tiles this context owns.  Returns the tensor."""
    return _OCCLUSION.into(self, tensor, _occlusion_params(first_frame, n_frames, rays, radius))


def _occlusion_samples(self, first_frame: int = 0, n_frames: int = 1, rays: int = 1, radius: float = 1.0) -> np.ndarray:
    """rene_occlusion_samples (probe): every ray occlusion() aggregates, a (n_frames, rays, yres, xres) structured array of
    abi.OCCLUSION_SAMPLE_DTYPE -- the first hit's position p and facing normal n, the two draws r1 and r2, the direction w and the state
    (abi.OCCLUSION_MISS, _OPEN, _OCCLUDED, _NO_RAY)."""
    out = np.zeros((max(int(n_frames), 0), max(int(rays), 0), self.yres, self.xres), abi.OCCLUSION_SAMPLE_DTYPE)
    _check(lib().rene_occlusion_samples(self._h, C.byref(_occlusion_params(first_frame, n_frames, rays, radius)), out.ctypes.data_as(C.c_void_p), out.size))
    return out


Renderer.occlusion = _occlusion
Renderer.occlusion_buffer = _OCCLUSION.buffer
Renderer.occlusion_into = _occlusion_into
Renderer.occlusion_samples = _occlusion_samples


# ---- the direct-light pass (rene_direct): the path estimator's first two steps, per pixel ----------------------------------------------------------
def _direct_params(first_frame, n_frames) -> abi.DirectParams:
    p = direct_params_default()
    p.first_frame, p.n_frames = first_frame, n_frames
    return p


def _direct(self, first_frame: int = 0, n_frames: int = 16) -> np.ndarray:
    """rene_direct into the library's own device buffer, downloaded: a (yres, xres) structured array of abi.DIRECT_DTYPE -- per pixel, over frames
    first_frame .. first_frame + n_frames - 1 and from the job's own seeds, the sums of what the primary ray saw (`seen`), of the distant lights
    (`distant`) and of what the light / BSDF mixture ray found (`sampled`), with hits and n.  direct_sum() and direct_mean() turn the records
    into images, indirect_mean() into the indirect light of the same samples.  Nothing of the accumulated image is read or changed.  Pixels of
    tiles the context does not own are the all-zero record (n == 0): direct_merge() joins the tile shards' arrays."""
    return _DIRECT.run(self, _direct_params(first_frame, n_frames))


def _direct_into(self, tensor, first_frame: int = 0, n_frames: int = 16):
    """rene_direct into a caller-owned torch tensor on the context's device: contiguous, uint8 or int32, yres * xres * 48 bytes (any shape).  All
    of it is written: zeros, then the records of the tiles this context owns.  Returns the tensor."""
    return _DIRECT.into(self, tensor, _direct_params(first_frame, n_frames))


def _direct_samples(self, first_frame: int = 0, n_frames: int = 1) -> np.ndarray:
    """rene_direct_samples (probe): every sample direct() aggregates, a (n_frames, yres, xres) structured array of abi.DIRECT_SAMPLE_DTYPE -- the
    three contributions, the mixture ray's direction wi and pdf, the state (abi.DIRECT_MISS, _LIGHT, _BSDF, _PLAIN, _ENDED_PDF, _ENDED_ZERO) and
    what the second query found (abi.DIRECT_SECOND_*)."""
    out = np.zeros((max(int(n_frames), 0), self.yres, self.xres), abi.DIRECT_SAMPLE_DTYPE)
    _check(lib().rene_direct_samples(self._h, C.byref(_direct_params(first_frame, n_frames)), out.ctypes.data_as(C.c_void_p), out.size))
    return out


Renderer.direct = _direct
Renderer.direct_buffer = _DIRECT.buffer
Renderer.direct_into = _direct_into
Renderer.direct_samples = _direct_samples


# ---- the bounce pass (rene_bounces): a job's radiance split by path depth, per pixel ---------------------------------------------------------------
def _bounces_params(first_frame, n_frames, max_depth) -> abi.BouncesParams:
    p = bounces_params_default()
    p.first_frame, p.n_frames, p.max_depth = first_frame, n_frames, max_depth
    return p


def _bounces(self, first_frame: int = 0, n_frames: int = 16, max_depth: int = 0) -> np.ndarray:
    """rene_bounces into the library's own device buffer, downloaded: a (yres, xres) structured array of abi.BOUNCES_DTYPE -- per pixel, over frames
    first_frame .. first_frame + n_frames - 1 and from the job's own seeds, the whole path estimator's radiance split by the iteration that added
    it (`bucket`[d]["sum"], d = 0 .. 8, and 9 for every iteration from 9 on, with `reached`), the paths' lengths (length_sum, length_max) and the
    samples the cap ended (capped), with n.  max_depth caps a path's iterations (1 .. 50; 0: rene's own 50).  bounces_sum(), bounces_depth_mean(),
    bounces_mean_length() and bounces_reached() turn the records into images.  Nothing of the accumulated image is read or changed.  Pixels of
    tiles the context does not own are the all-zero record (n == 0): bounces_merge() joins the tile shards' arrays."""
    return _BOUNCES.run(self, _bounces_params(first_frame, n_frames, max_depth))


def _bounces_into(self, tensor, first_frame: int = 0, n_frames: int = 16, max_depth: int = 0):
    """rene_bounces into a caller-owned torch tensor on the context's device: contiguous, uint8 or int32, yres * xres * 176 bytes (any shape).  All
    of it is written: zeros, then the records of the tiles this context owns.  Returns the tensor."""
    return _BOUNCES.into(self, tensor, _bounces_params(first_frame, n_frames, max_depth))


def _bounces_samples(self, first_frame: int = 0, n_frames: int = 1, max_depth: int = 0) -> np.ndarray:
    """rene_bounces_samples (probe): every sample bounces() aggregates, a (n_frames, yres, xres) structured array of abi.BOUNCES_SAMPLE_DTYPE -- the
    ten values and counts of the sample, its length and how it ended (abi.BOUNCES_END_MISS, _PDF, _ZERO, _ROULETTE, _CAP)."""
    out = np.zeros((max(int(n_frames), 0), self.yres, self.xres), abi.BOUNCES_SAMPLE_DTYPE)
    _check(lib().rene_bounces_samples(self._h, C.byref(_bounces_params(first_frame, n_frames, max_depth)), out.ctypes.data_as(C.c_void_p), out.size))
    return out


Renderer.bounces = _bounces
Renderer.bounces_buffer = _BOUNCES.buffer
Renderer.bounces_into = _bounces_into
Renderer.bounces_samples = _bounces_samples


# ---- the light-group pass (rene_lights): a job's radiance split by the light it came from, per pixel ----------------------------------------------
def _lights_params(first_frame, n_frames, groups):
    """The call's params and what keeps its tables alive: `groups` is None (the library's grouping) or (instance_group, distant_group,
    background_group), one group below 8 per instance and per distant light of the scene."""
    p = lights_params_default()
    p.first_frame, p.n_frames = first_frame, n_frames
    if groups is None:
        return p, ()
    inst, dist, bg = groups
    inst, dist = np.ascontiguousarray(inst, np.uint8).reshape(-1), np.ascontiguousarray(dist, np.uint8).reshape(-1)
    if not 0 <= int(bg) <= 255:
        raise ValueError("lights(): background_group must be 0 .. 7")
    p.n_instances, p.n_distant, p.background_group = inst.size, dist.size, int(bg)
    p.instance_group = inst.ctypes.data if inst.size else None
    p.distant_group = dist.ctypes.data if dist.size else None
    if not inst.size and not dist.size:  # (a scene without sources in a table: params without tables would name the library's grouping)
        inst = np.zeros(1, np.uint8)
        p.instance_group = inst.ctypes.data
    return p, (inst, dist)


def _lights(self, first_frame: int = 0, n_frames: int = 16, groups=None) -> np.ndarray:
    """rene_lights into the library's own device buffer, downloaded: a (yres, xres) structured array of abi.LIGHTS_DTYPE -- per pixel, over frames
    first_frame .. first_frame + n_frames - 1 and from the job's own seeds, the whole path estimator's radiance split by the SOURCE of each add
    into eight groups (`group`[g]["sum"], with `adds`, the adds that were not black), with n and lit (the samples with any such add).  groups:
    (instance_group, distant_group, background_group) -- one group below 8 per instance of the scene (read for instances with an area light), per
    distant light, and for the background -- or None for the library's grouping, light_groups().  lights_sum(), lights_group_sum(),
    lights_group_mean() and lights_mix() turn the records into images.  Nothing of the accumulated image is read or changed.  Pixels of tiles
    the context does not own are the all-zero record (n == 0): lights_merge() joins the tile shards' arrays."""
    p, keep = _lights_params(first_frame, n_frames, groups)
    out = _LIGHTS.run(self, p)
    del keep
    return out


def _lights_into(self, tensor, first_frame: int = 0, n_frames: int = 16, groups=None):
    """rene_lights into a caller-owned torch tensor on the context's device: contiguous, uint8 or int32, yres * xres * 144 bytes (any shape).  All
    of it is written: zeros, then the records of the tiles this context owns.  Returns the tensor."""
    p, keep = _lights_params(first_frame, n_frames, groups)
    out = _LIGHTS.into(self, tensor, p)
    del keep
    return out


def _lights_samples(self, first_frame: int = 0, n_frames: int = 1, groups=None) -> np.ndarray:
    """rene_lights_samples (probe): every sample lights() aggregates, a (n_frames, yres, xres) structured array of abi.LIGHTS_SAMPLE_DTYPE -- the
    eight values and counts of the sample, whether it is lit, its length and how it ended (abi.BOUNCES_END_*)."""
    p, keep = _lights_params(first_frame, n_frames, groups)
    out = np.zeros((max(int(n_frames), 0), self.yres, self.xres), abi.LIGHTS_SAMPLE_DTYPE)
    _check(lib().rene_lights_samples(self._h, C.byref(p), out.ctypes.data_as(C.c_void_p), out.size))
    del keep
    return out


def _light_groups(self):
    """rene_lights_default_groups: ((instance_group, distant_group, background_group), n_used) -- the library's grouping of the scene, uint8 arrays
    over its instances and its distant lights.  Group 0 is the background, then a group per distant light in table order, then one per instance
    with an area light in instance order; what does not fit shares group 7; instances without an area light get 0 (they never add)."""
    inst, dist = np.zeros(self._packed.desc.n_instances, np.uint8), np.zeros(self._packed.desc.n_lights, np.uint8)
    bg, used = C.c_uint8(), C.c_uint32()
    _check(lib().rene_lights_default_groups(self._h, inst.ctypes.data if inst.size else None, inst.size, dist.ctypes.data if dist.size else None, dist.size,
                                            C.byref(bg), C.byref(used)))
    return (inst, dist, int(bg.value)), int(used.value)


Renderer.lights = _lights
Renderer.lights_buffer = _LIGHTS.buffer
Renderer.lights_into = _lights_into
Renderer.lights_samples = _lights_samples
Renderer.light_groups = _light_groups


# ---- multi-channel OpenEXR output (include/rene_hip.h: rene_output_exr) ---------------------------------------------------------------------------
_EXR_LAYERS = {"beauty": abi.EXR_BEAUTY, "albedo": abi.EXR_ALBEDO, "normal": abi.EXR_NORMAL, "denoised": abi.EXR_DENOISED, "alpha": abi.EXR_ALPHA,
               "depth": abi.EXR_DEPTH, "position": abi.EXR_POSITION, "ids": abi.EXR_IDS}
_EXR_BEAUTY = {"radiance": abi.OUTPUT_RADIANCE, "denoised_mean": abi.OUTPUT_DENOISED_MEAN, "robust": abi.OUTPUT_ROBUST}


def exr_mask(layers) -> int:
    """The RENE_EXR_* mask of layer names ("beauty", "albedo", "normal", "denoised", "alpha", "depth", "position", "ids"), or the mask itself."""
    if isinstance(layers, int):
        return layers
    if isinstance(layers, str):
        layers = (layers,)
    mask = 0
    for name in layers:
        if name not in _EXR_LAYERS:
            raise ValueError(f"layers must be among {sorted(_EXR_LAYERS)}, not {name!r}")
        mask |= _EXR_LAYERS[name]
    return mask


def exr_params_default() -> abi.ExrParams:
    """rene_exr_params_default: BEAUTY | ALBEDO | NORMAL, RADIANCE (host only)."""
    p = abi.ExrParams()
    lib().rene_exr_params_default(C.byref(p))
    return p


def _exr_params(layers, beauty) -> abi.ExrParams:
    if beauty not in _EXR_BEAUTY:
        raise ValueError(f"beauty must be one of {sorted(_EXR_BEAUTY)}, not {beauty!r}")
    p = exr_params_default()
    p.layers, p.beauty_source = exr_mask(layers), _EXR_BEAUTY[beauty]
    return p


def exr_layout(xres: int, yres: int, layers=("beauty", "albedo", "normal")) -> tuple[int, int, int]:
    """rene_exr_layout: (header bytes with the offset table, body bytes, bytes per pixel) of an xres x yres file of `layers` (host only)."""
    head, body, bpp = C.c_size_t(), C.c_size_t(), C.c_uint32()
    _check(lib().rene_exr_layout(xres, yres, exr_mask(layers), C.byref(head), C.byref(body), C.byref(bpp)))
    return head.value, body.value, bpp.value


def exr_header(xres: int, yres: int, layers=("beauty", "albedo", "normal")) -> bytes:
    """rene_exr_header: the header and the offset table of an xres x yres file of `layers` (host only); the body follows it."""
    head = exr_layout(xres, yres, layers)[0]
    buf = C.create_string_buffer(head)
    _check(lib().rene_exr_header(xres, yres, exr_mask(layers), buf, head))
    return buf.raw


def exr_body_host(xres: int, yres: int, layers, *, beauty=None, albedo=None, normal=None, denoised=None, alpha=None, depth=None, position=None,
                  ids=None, coverage=None) -> bytes:
    """rene_exr_body_host: the body of a file of `layers` packed on the host from planes of means -- (yres, xres, 3) float32 for beauty, albedo,
    normal, denoised and position, (yres, xres) for alpha and depth, (yres, xres, 4) uint32 ids and float32 coverage."""
    keep = []

    def ptr(a, dtype, shape):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype)
        if a.shape != shape:
            raise ValueError(f"a plane of shape {a.shape} where the film's is {shape}")
        keep.append(a)
        return a.ctypes.data

    p = abi.ExrPlanes()
    p.struct_size = C.sizeof(abi.ExrPlanes)
    rgb, one, four = (yres, xres, 3), (yres, xres), (yres, xres, 4)
    p.beauty, p.albedo, p.normal, p.denoised = ptr(beauty, np.float32, rgb), ptr(albedo, np.float32, rgb), ptr(normal, np.float32, rgb), ptr(denoised, np.float32, rgb)
    p.alpha, p.depth, p.position = ptr(alpha, np.float32, one), ptr(depth, np.float32, one), ptr(position, np.float32, rgb)
    p.ids, p.coverage = ptr(ids, np.uint32, four), ptr(coverage, np.float32, four)
    mask = exr_mask(layers)
    body = exr_layout(xres, yres, mask)[1]
    buf = C.create_string_buffer(body)
    _check(lib().rene_exr_body_host(xres, yres, mask, C.byref(p), buf, body))
    return buf.raw


_EXR_COMPRESSION = {"none": abi.EXR_COMPRESSION_NONE, "zips": abi.EXR_COMPRESSION_ZIPS}


def exr_compression(compression) -> int:
    """The file format's code of "none" or "zips", or the code itself (checked by the library)."""
    if isinstance(compression, str):
        if compression not in _EXR_COMPRESSION:
            raise ValueError(f"compression must be one of {sorted(_EXR_COMPRESSION)}, not {compression!r}")
        return _EXR_COMPRESSION[compression]
    return int(compression)


def exr_tail_bound(xres: int, yres: int, layers=("beauty", "albedo", "normal")) -> int:
    """rene_exr_tail_bound: the most bytes a compressed file's tail -- offset table and chunks -- takes (host only)."""
    exr_layout(xres, yres, layers)  # (raises on a bad mask or film)
    return lib().rene_exr_tail_bound(xres, yres, exr_mask(layers))


def exr_attributes(xres: int, yres: int, layers=("beauty", "albedo", "normal"), compression="zips") -> bytes:
    """rene_exr_attributes: the file from the magic through the header's terminating 0, with the compression attribute set (host only); the tail
    follows it."""
    mask = exr_mask(layers)
    n = exr_layout(xres, yres, mask)[0] - 8 * yres
    buf = C.create_string_buffer(n)
    _check(lib().rene_exr_attributes(xres, yres, mask, exr_compression(compression), buf, n))
    return buf.raw


def exr_compress_host(xres: int, yres: int, layers, body, compression="zips") -> bytes:
    """rene_exr_compress_host: the tail of an xres x yres file of `layers` from its uncompressed body (bytes, or a uint8 array), on the host: the
    definition the device is held to.  The file is exr_attributes() + these bytes."""
    mask = exr_mask(layers)
    body = np.ascontiguousarray(np.frombuffer(body, np.uint8) if isinstance(body, (bytes, bytearray, memoryview)) else np.asarray(body, np.uint8))
    bound = lib().rene_exr_tail_bound(xres, yres, mask) or 16
    out, written = np.empty(bound, np.uint8), C.c_size_t()
    _check(lib().rene_exr_compress_host(xres, yres, mask, exr_compression(compression), body.ctypes.data_as(C.c_void_p), body.size,
                                        out.ctypes.data_as(C.c_void_p), out.size, C.byref(written)))
    return out[:written.value].tobytes()


def _download_exr_tail(self) -> bytes:
    """rene_download_exr_tail: tail[:written] of the last compression into the library's own buffer."""
    n = _result_buffer(self, lib().rene_exr_tail_buffer)[1]
    return _download_result(self, lib().rene_download_exr_tail, (n,), np.uint8).tobytes()


def _exr_compress(self, tensor, xres: int, yres: int, layers, body, compression="zips"):
    """rene_exr_compress: the tail of an xres x yres file of `layers` from `body`, a uint8 torch tensor on the context's device that holds the
    uncompressed body (exr_into's tensor, or one the tile shards of the device filled between them); the film need not be the context's.
    tensor: a uint8 tensor of at least exr_tail_bound() bytes -- returns (tensor, written), the file is exr_attributes() + tensor[:written], the
    bytes beyond stay as they were -- or None: the library's own buffer, downloaded -- returns the tail's bytes."""
    mask = exr_mask(layers)
    _check_tensor("exr_compress", body, self.device, ("uint8",), shape=(exr_layout(xres, yres, mask)[1],), what="body")
    written = C.c_size_t()
    if tensor is None:
        _check(lib().rene_exr_compress(self._h, xres, yres, mask, exr_compression(compression), C.c_void_p(body.data_ptr()), body.numel(), None, 0, C.byref(written)))
        return _download_exr_tail(self)
    _check_tensor("exr_compress", tensor, self.device, ("uint8",), what="tail")
    _check(lib().rene_exr_compress(self._h, xres, yres, mask, exr_compression(compression), C.c_void_p(body.data_ptr()), body.numel(),
                                   C.c_void_p(tensor.data_ptr()), tensor.numel(), C.byref(written)))
    return tensor, written.value


def _exr(self, path=None, layers=("beauty", "albedo", "normal"), beauty: str = "radiance", compression="none") -> bytes:
    """rene_output_exr into the library's own device buffer, downloaded behind its header: the bytes of a scan-line OpenEXR file with
    the channels of `layers` -- "beauty" (R G B: the mean of `beauty`, "radiance", "denoised_mean" or "robust"), "albedo", "normal", "denoised"
    (after a denoise call), and from the last gbuffer() "alpha" (A), "depth" (Z), "position" (P.X .Y .Z) and "ids" (id0 .. id3, cov0 .. cov3).
    compression: "none", or "zips" -- rene_output_exr_compressed: every scan line deflated on the device, a smaller file.
    Only the file's bytes cross PCIe.  Written to `path` too where one is given."""
    p = _exr_params(layers, beauty)
    code = exr_compression(compression)
    if code == abi.EXR_COMPRESSION_NONE:
        _check(lib().rene_output_exr(self._h, C.byref(p), None, 0))
        head, body, _ = exr_layout(self.xres, self.yres, p.layers)
        buf = np.empty(head + body, np.uint8)  # the header, and the body downloaded behind it: one copy to the bytes handed out
        _check(lib().rene_exr_header(self.xres, self.yres, p.layers, buf.ctypes.data_as(C.c_void_p), head))
        _check(lib().rene_download_exr(self._h, C.c_void_p(buf.ctypes.data + head), body))
    else:
        written = C.c_size_t()
        _check(lib().rene_output_exr_compressed(self._h, C.byref(p), code, None, 0, C.byref(written)))
        head = exr_layout(self.xres, self.yres, p.layers)[0] - 8 * self.yres
        buf = np.empty(head + written.value, np.uint8)  # the attributes, and tail[:written] downloaded behind them
        _check(lib().rene_exr_attributes(self.xres, self.yres, p.layers, code, buf.ctypes.data_as(C.c_void_p), head))
        _check(lib().rene_download_exr_tail(self._h, C.c_void_p(buf.ctypes.data + head), written.value))
    if path is not None:
        with open(path, "wb") as f:
            f.write(buf.data)
    return buf.tobytes()


def _exr_buffer(self):
    """rene_exr_buffer: (device pointer, bytes) of the last exr() body."""
    return _result_buffer(self, lib().rene_exr_buffer)


def _exr_into(self, tensor, layers=("beauty", "albedo", "normal"), beauty: str = "radiance", compression="none"):
    """rene_output_exr into a caller-owned torch tensor on the context's device: contiguous, uint8, of the body's size (exr_layout).  Only the bytes
    of the tiles this context owns are written, and the prefix of their rows, so the tile shards of one device fill one tensor between them; the
    file is exr_header() + the tensor's bytes.  Returns the tensor.
    compression="zips" (or "none" through the same call): rene_output_exr_compressed into a tensor of at least exr_tail_bound() bytes; returns
    (tensor, written), and the file is exr_attributes() + tensor[:written]."""
    p = _exr_params(layers, beauty)
    if isinstance(compression, str) and compression == "none":
        _check_tensor("exr_into", tensor, self.device, ("uint8",), shape=(exr_layout(self.xres, self.yres, p.layers)[1],), what="body")
        _check(lib().rene_output_exr(self._h, C.byref(p), C.c_void_p(tensor.data_ptr()), tensor.numel()))
        return tensor
    _check_tensor("exr_into", tensor, self.device, ("uint8",), what="tail")
    written = C.c_size_t()
    _check(lib().rene_output_exr_compressed(self._h, C.byref(p), exr_compression(compression), C.c_void_p(tensor.data_ptr()), tensor.numel(), C.byref(written)))
    return tensor, written.value


Renderer.exr = _exr
Renderer.exr_buffer = _exr_buffer
Renderer.exr_into = _exr_into
Renderer.exr_compress = _exr_compress
Renderer.download_exr_tail = _download_exr_tail


# ---- Cryptomatte output (include/rene_hip.h: rene_output_cryptomatte) -----------------------------------------------------------------------------
# a layer as cryptomatte() names it: the file's layer name, the ids its records hold (gbuffer()'s `ids`), where a scene keeps the names
_CRYPTOMATTE_LAYERS = {"object": ("CryptoObject", "instance", "instance_names"), "material": ("CryptoMaterial", "material", "material_names")}


def cryptomatte_hash(name) -> int:
    """rene_cryptomatte_hash: MurmurHash3_x86_32 of the name's UTF-8 bytes (or of bytes), seed 0, with the exponent fix that keeps the id a normal
    float; the result is the FLOAT channel's bit pattern (host only)."""
    data = name.encode() if isinstance(name, str) else bytes(name)
    return int(lib().rene_cryptomatte_hash(data, len(data)))


def _c_names(names):
    """A list of names as a char*[] (and the list, which owns the bytes)."""
    data = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    if any(b"\0" in d for d in data):
        raise ValueError("a name holds a 0 byte")
    return (C.c_char_p * max(1, len(data)))(*data), data


def cryptomatte_manifest(names) -> str:
    """rene_cryptomatte_manifest: {"<name>":"<%08x of its hash>",...} of the distinct names, ordered by their bytes (host only)."""
    arr, keep = _c_names(names)
    n = C.c_size_t()
    _check(lib().rene_cryptomatte_manifest(arr, len(keep), None, 0, C.byref(n)))
    buf = C.create_string_buffer(max(1, n.value))
    _check(lib().rene_cryptomatte_manifest(arr, len(keep), buf, n.value, C.byref(n)))
    return buf.raw[:n.value].decode(errors="surrogateescape")


def _cryptomatte_layers(layers):
    """[(layer name, "instance" | "material", names, records pointer or None), ...] as an array of abi.CryptomatteLayer, and what it points at."""
    keep, out = [], (abi.CryptomatteLayer * max(1, len(layers)))()
    for k, (name, ids, names, records) in enumerate(layers):
        if ids not in ("instance", "material"):
            raise ValueError(f"a Cryptomatte layer's ids are 'instance' or 'material', not {ids!r}")
        arr, data = _c_names(names)
        keep += [arr, data]
        out[k].name, out[k].id_source, out[k].n_names = name.encode(), _GBUFFER_IDS[ids], len(data)
        out[k].names, out[k].records = arr, records
    return out, keep


def _cryptomatte_host_layers(layers):
    return _cryptomatte_layers([(name, ids, names, None) for name, ids, names in layers])


def cryptomatte_layout(xres: int, yres: int, layers) -> tuple[int, int, int]:
    """rene_cryptomatte_layout: (attribute bytes, body bytes, bytes per pixel) of an xres x yres file of `layers`, a list of
    (layer name, "instance" | "material", names) (host only).  The uncompressed file is attributes + 8 * yres of table + body."""
    arr, keep = _cryptomatte_host_layers(layers)
    head, body, bpp = C.c_size_t(), C.c_size_t(), C.c_uint32()
    _check(lib().rene_cryptomatte_layout(xres, yres, arr, len(layers), C.byref(head), C.byref(body), C.byref(bpp)))
    return head.value, body.value, bpp.value


def cryptomatte_attributes(xres: int, yres: int, layers, compression="zips") -> bytes:
    """rene_cryptomatte_attributes: the file from the magic through the header's terminating 0 -- the channel list, the eight attributes of every
    file of this library's and the four cryptomatte/<key>/* strings of every layer (host only)."""
    arr, keep = _cryptomatte_host_layers(layers)
    n = cryptomatte_layout(xres, yres, layers)[0]
    buf = C.create_string_buffer(n)
    _check(lib().rene_cryptomatte_attributes(xres, yres, arr, len(layers), exr_compression(compression), buf, n))
    return buf.raw


def cryptomatte_body_host(xres: int, yres: int, layers, records) -> bytes:
    """rene_cryptomatte_body_host: the body packed on the host from one (yres, xres) array of abi.GBUFFER_DTYPE records per layer: the definition
    the device is held to."""
    arr, keep = _cryptomatte_host_layers(layers)
    recs = [np.ascontiguousarray(_gbuffer_records(r)) for r in records]
    if len(recs) != len(layers) or any(r.shape != (yres, xres) for r in recs):
        raise ValueError("cryptomatte_body_host() takes one (yres, xres) record array per layer")
    ptrs = (C.c_void_p * max(1, len(recs)))(*[r.ctypes.data for r in recs])
    body = cryptomatte_layout(xres, yres, layers)[1]
    buf = C.create_string_buffer(body)
    _check(lib().rene_cryptomatte_body_host(xres, yres, arr, len(layers), ptrs, buf, body))
    return buf.raw


def exr_compress_rows_host(row_bytes: int, yres: int, attributes_bytes: int, body, compression="zips") -> bytes:
    """rene_exr_compress_rows_host: the tail -- offset table and chunks -- of a file of yres rows of row_bytes behind attributes_bytes of
    attributes, from its uncompressed body, on the host."""
    body = np.ascontiguousarray(np.frombuffer(body, np.uint8) if isinstance(body, (bytes, bytearray, memoryview)) else np.asarray(body, np.uint8))
    out, written = np.empty(max(16, 8 * yres + body.size), np.uint8), C.c_size_t()
    _check(lib().rene_exr_compress_rows_host(row_bytes, yres, attributes_bytes, exr_compression(compression), body.ctypes.data_as(C.c_void_p), body.size,
                                             out.ctypes.data_as(C.c_void_p), out.size, C.byref(written)))
    return out[:written.value].tobytes()


def _exr_compress_rows(self, row_bytes: int, yres: int, attributes_bytes: int, body, compression="zips") -> bytes:
    """rene_exr_compress_rows into the library's own buffer, downloaded: the tail of a file of yres rows of row_bytes from `body`, a uint8 torch
    tensor on the context's device (cryptomatte_into's, say, which the tile shards of the device filled between them)."""
    _check_tensor("exr_compress_rows", body, self.device, ("uint8",), shape=(yres * (8 + row_bytes),), what="body")
    written = C.c_size_t()
    _check(lib().rene_exr_compress_rows(self._h, row_bytes, yres, attributes_bytes, exr_compression(compression), C.c_void_p(body.data_ptr()), body.numel(),
                                        None, 0, C.byref(written)))
    return _download_exr_tail(self)


def _cryptomatte_names(self, layer, names):
    if names is not None and layer in names:
        return list(names[layer])
    getter = getattr(self._scene, _CRYPTOMATTE_LAYERS[layer][2], None)
    if getter is None:
        raise ValueError(f"the scene this Renderer was made from has no names; pass names={{{layer!r}: [...]}}")
    return getter()


def cryptomatte_scene_layers(layers, names_of) -> list:
    """The (layer name, ids, names) list of `layers` ("object", "material") with names_of(layer) as each one's names: what the host-only
    functions above take for the file Renderer.cryptomatte() writes."""
    layers = (layers,) if isinstance(layers, str) else tuple(layers)
    for layer in layers:
        if layer not in _CRYPTOMATTE_LAYERS:
            raise ValueError(f"layers must be among {sorted(_CRYPTOMATTE_LAYERS)}, not {layer!r}")
    return [(_CRYPTOMATTE_LAYERS[layer][0], _CRYPTOMATTE_LAYERS[layer][1], names_of(layer)) for layer in layers]


def _output_cryptomatte(self, layers, tensor=None, download=True):
    """rene_output_cryptomatte of `layers`, a list of (layer name, "instance" | "material", names, records): records is a uint8 torch tensor on the
    context's device that holds the layer's geometry records (gbuffer_into's), or None for the library-owned result of the last gbuffer().
    tensor: the caller-owned uint8 destination (returned), or None: the library's own buffer, whose bytes are returned (download=False: None)."""
    for _, _, _, rec in layers:
        if rec is not None:
            _check_tensor("output_cryptomatte", rec, self.device, ("uint8",), numel=gbuffer_bytes(self.xres, self.yres))
    arr, keep = _cryptomatte_layers([(n, i, l, None if r is None else r.data_ptr()) for n, i, l, r in layers])
    p = abi.CryptomatteParams()
    lib().rene_cryptomatte_params_default(C.byref(p))
    p.n_layers, p.layers = len(layers), arr
    if tensor is not None:
        _check_tensor("output_cryptomatte", tensor, self.device, ("uint8",), what="body")
        _check(lib().rene_output_cryptomatte(self._h, C.byref(p), C.c_void_p(tensor.data_ptr()), tensor.numel()))
        return tensor
    _check(lib().rene_output_cryptomatte(self._h, C.byref(p), None, 0))
    if not download:
        return None
    n = _result_buffer(self, lib().rene_cryptomatte_buffer)[1]
    return _download_result(self, lib().rene_download_cryptomatte, (n,), np.uint8).tobytes()


def _cryptomatte_pack(self, tensor, layers, first_frame, n_frames, names):
    """One gbuffer() per layer -- the first into the library's buffer, the others into torch tensors -- then rene_output_cryptomatte into `tensor`
    or, with None, into the library's buffer.  Returns the (layer name, ids, names) list."""
    described = cryptomatte_scene_layers(layers, lambda layer: _cryptomatte_names(self, layer, names))
    if not described:
        raise ValueError("cryptomatte() takes at least one layer")
    full = []
    for k, (name, ids, layer_names) in enumerate(described):
        p = _gbuffer_params(first_frame, n_frames, ids)
        if k == 0:
            _check(lib().rene_gbuffer(self._h, C.byref(p), None, 0))
            full.append((name, ids, layer_names, None))
        else:
            import torch
            rec = torch.empty(gbuffer_bytes(self.xres, self.yres), dtype=torch.uint8, device=f"cuda:{self.device}")
            _GBUFFER.into(self, rec, p)
            full.append((name, ids, layer_names, rec))
    _output_cryptomatte(self, full, tensor, download=False)
    return described


def _cryptomatte(self, path=None, layers=("object", "material"), first_frame: int = 0, n_frames: int = 16, compression="zips", names=None) -> bytes:
    """A Cryptomatte file of the scene's id mattes by NAME, the format Nuke, Fusion, Blender and Natron read: the geometry pass over frames
    first_frame .. first_frame + n_frames - 1 once per layer -- "object" (CryptoObject: instances) and / or "material" (CryptoMaterial) -- packed
    on the device (rene_output_cryptomatte) and, with compression "zips", deflated there (rene_exr_compress_rows).  The names are the Scene's
    (instance_names(), material_names()) unless names={"object": [...], ...} gives a list of the caller's over the instances or materials: ids of
    one name are one matte.  Returns the file's bytes; written to `path` too (through path + ".tmp") where one is given."""
    code = exr_compression(compression)
    if self._shard_count > 1:
        raise ReneError(-4, "cryptomatte(): a row spans tiles of several shards; fill one body with cryptomatte_into() and compress it with exr_compress_rows()")
    described = _cryptomatte_pack(self, None, layers, first_frame, n_frames, names)
    attributes = cryptomatte_attributes(self.xres, self.yres, described, code)
    body_ptr, body_bytes = _result_buffer(self, lib().rene_cryptomatte_buffer)
    written = C.c_size_t()
    _check(lib().rene_exr_compress_rows(self._h, (body_bytes // self.yres) - 8, self.yres, len(attributes), code, C.c_void_p(body_ptr), body_bytes, None, 0,
                                        C.byref(written)))
    data = attributes + _download_exr_tail(self)
    if path is not None:
        tmp = str(path) + ".tmp"
        with open(tmp, "wb") as f:
            f.write(data)
        os.replace(tmp, path)
    return data


def _cryptomatte_into(self, tensor, layers=("object", "material"), first_frame: int = 0, n_frames: int = 16, names=None):
    """rene_output_cryptomatte into a caller-owned torch tensor on the context's device: contiguous, uint8, of the body's size
    (cryptomatte_layout).  Only the bytes of the tiles this context owns are written, and the prefix of their rows, so the tile shards of one
    device fill one tensor between them; the file is cryptomatte_attributes() + the table + the tensor's bytes, or exr_compress_rows() of
    them.  Returns the tensor."""
    described = cryptomatte_scene_layers(layers, lambda layer: _cryptomatte_names(self, layer, names))
    _check_tensor("cryptomatte_into", tensor, self.device, ("uint8",), shape=(cryptomatte_layout(self.xres, self.yres, described)[1],), what="body")
    _cryptomatte_pack(self, tensor, layers, first_frame, n_frames, names)
    return tensor


def _cryptomatte_buffer(self):
    """rene_cryptomatte_buffer: (device pointer, bytes) of the last body packed into the library's own buffer."""
    return _result_buffer(self, lib().rene_cryptomatte_buffer)


Renderer.cryptomatte = _cryptomatte
Renderer.cryptomatte_into = _cryptomatte_into
Renderer.cryptomatte_buffer = _cryptomatte_buffer
Renderer.output_cryptomatte = _output_cryptomatte
Renderer.exr_compress_rows = _exr_compress_rows


def gbuffer_depth(rec) -> np.ndarray:
    """The mean depth of the hitting samples, depth_sum / hits in fp32; +inf where nothing hit."""
    rec = _gbuffer_records(rec)
    hit = rec["hits"] > 0
    out = np.full(rec.shape, np.inf, np.float32)
    out[hit] = rec["depth_sum"][hit] / rec["hits"][hit].astype(np.float32)
    return out


def gbuffer_coverage(rec) -> np.ndarray:
    """hits / n in fp32 (0 where n == 0): the alpha of the geometry against the background."""
    rec = _gbuffer_records(rec)
    out = np.zeros(rec.shape, np.float32)
    own = rec["n"] > 0
    out[own] = rec["hits"][own].astype(np.float32) / rec["n"][own].astype(np.float32)
    return out


def gbuffer_position(rec) -> np.ndarray:
    """The mean world position of the hitting samples, position_sum / hits in fp32, (..., 3); 0 where nothing hit."""
    rec = _gbuffer_records(rec)
    out = np.zeros(rec.shape + (3,), np.float32)
    hit = rec["hits"] > 0
    out[hit] = rec["position_sum"][hit] / rec["hits"][hit].astype(np.float32)[:, None]
    return out


def gbuffer_matte(rec, id: int) -> np.ndarray:
    """count / n of one id in fp32: its anti-aliased matte (0 where the id holds no slot; samples counted in `other` are in no matte)."""
    rec = _gbuffer_records(rec)
    count = np.where((rec["id"] == np.uint32(id)) & (rec["count"] > 0), rec["count"], 0).sum(axis=-1)
    out = np.zeros(rec.shape, np.float32)
    own = rec["n"] > 0
    out[own] = count[own].astype(np.float32) / rec["n"][own].astype(np.float32)
    return out


def occlusion_ao(rec) -> np.ndarray:
    """The ambient occlusion, 1 - occluded / rays in fp32; 1 where no ray was cast."""
    rec = _occlusion_records(rec)
    out = np.ones(rec.shape, np.float32)
    cast = rec["rays"] > 0
    out[cast] = np.float32(1.0) - rec["occluded"][cast].astype(np.float32) / rec["rays"][cast].astype(np.float32)
    return out


def occlusion_bent(rec) -> np.ndarray:
    """The bent normal, bent_sum / |bent_sum| in fp32, (..., 3); 0 where bent_sum is 0."""
    rec = _occlusion_records(rec)
    b = rec["bent_sum"]
    length = np.sqrt(b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1] + b[..., 2] * b[..., 2])
    out = np.zeros(rec.shape + (3,), np.float32)
    some = length > 0
    out[some] = b[some] / length[some][:, None]
    return out


def direct_sum(rec) -> np.ndarray:
    """The direct light as a sum over the pass's frames, (..., 3): (seen + distant) + sampled in fp32, in that order."""
    rec = _direct_records(rec)
    return (rec["seen"].astype(np.float32) + rec["distant"].astype(np.float32)) + rec["sampled"].astype(np.float32)


def direct_mean(rec) -> np.ndarray:
    """The direct light per sample, direct_sum / n in fp32, (..., 3); 0 where n == 0 (a pixel no part owns)."""
    rec = _direct_records(rec)
    out = np.zeros(rec.shape + (3,), np.float32)
    own = rec["n"] != 0
    out[own] = direct_sum(rec)[own] / rec["n"][own].astype(np.float32)[:, None]
    return out


def indirect_mean(beauty_sum, rec) -> np.ndarray:
    """The indirect light per sample, (beauty_sum - direct_sum) / n in fp32, (..., 3): beauty_sum is the radiance layer as a SUM over the frames the
    pass ran over (download(0)[..., :3] of a context that rendered exactly those frames), so that both are sums over the same samples.  0 where
    n == 0."""
    rec = _direct_records(rec)
    beauty_sum = np.asarray(beauty_sum, np.float32)[..., :3]
    if beauty_sum.shape != rec.shape + (3,):
        raise ValueError("indirect_mean(): beauty_sum must be (..., 3) or (..., 4) over the records' shape")
    out = np.zeros(rec.shape + (3,), np.float32)
    own = rec["n"] != 0
    out[own] = (beauty_sum[own] - direct_sum(rec)[own]) / rec["n"][own].astype(np.float32)[:, None]
    return out


def bounces_sum(rec, upto: int = 10) -> np.ndarray:
    """The radiance of the pass's frames as a sum, (..., 3): the first `upto` buckets added from the left in fp32, ((b0 + b1) + b2) + ...  With
    upto = 10 that is the whole (capped) estimator; with upto = k <= 9 the estimator under a cap of k iterations."""
    rec = _bounces_records(rec)
    if not 0 <= int(upto) <= abi.BOUNCES_BUCKETS:
        raise ValueError("bounces_sum(): upto must be 0 .. 10")
    sums = rec["bucket"]["sum"].astype(np.float32)
    out = np.zeros(rec.shape + (3,), np.float32)  # (+ 0 + b0 is b0: no sum of the pass is ever - 0)
    for d in range(int(upto)):
        out = out + sums[..., d, :]
    return out


def _bounces_per_sample(rec, total) -> np.ndarray:
    out = np.zeros(total.shape, np.float32)
    own = rec["n"] != 0
    n = rec["n"][own].astype(np.float32)
    out[own] = total[own] / (n[:, None] if total.ndim > rec.ndim else n)
    return out


def bounces_depth_mean(rec, d: int) -> np.ndarray:
    """What iteration d (9: every iteration from 9 on) added per sample, bucket[d].sum / n in fp32, (..., 3); 0 where n == 0."""
    rec = _bounces_records(rec)
    if not 0 <= int(d) < abi.BOUNCES_BUCKETS:
        raise ValueError("bounces_depth_mean(): d must be 0 .. 9")
    return _bounces_per_sample(rec, rec["bucket"]["sum"][..., int(d), :].astype(np.float32))


def bounces_mean_length(rec) -> np.ndarray:
    """The mean path length, length_sum / n in fp32 (both converted first), (...); 0 where n == 0."""
    rec = _bounces_records(rec)
    return _bounces_per_sample(rec, rec["length_sum"].astype(np.float32))


def bounces_reached(rec) -> np.ndarray:
    """How many of the pixel's iterations fell into each bucket, (..., 10) uint32."""
    return _bounces_records(rec)["bucket"]["reached"].copy()


def _lights_group(name, g) -> int:
    if not 0 <= int(g) < abi.LIGHTS_GROUPS:
        raise ValueError(f"{name}(): g must be 0 .. 7")
    return int(g)


def lights_group_sum(rec, g: int) -> np.ndarray:
    """What the sources of group g added over the pass's frames, group[g].sum, (..., 3) fp32."""
    rec = _lights_records(rec)
    return rec["group"]["sum"][..., _lights_group("lights_group_sum", g), :].astype(np.float32)


def lights_group_mean(rec, g: int) -> np.ndarray:
    """What the sources of group g added per sample, group[g].sum / n in fp32, (..., 3); 0 where n == 0."""
    rec = _lights_records(rec)
    return _bounces_per_sample(rec, rec["group"]["sum"][..., _lights_group("lights_group_mean", g), :].astype(np.float32))


def lights_sum(rec) -> np.ndarray:
    """The radiance of the pass's frames as a sum, (..., 3): the eight groups added from the left in fp32, ((g0 + g1) + g2) + ..."""
    rec = _lights_records(rec)
    sums = rec["group"]["sum"].astype(np.float32)
    out = sums[..., 0, :].copy()
    for g in range(1, abi.LIGHTS_GROUPS):
        out = out + sums[..., g, :]
    return out


def lights_mix(rec, weights) -> np.ndarray:
    """The relit mean image, (..., 3) fp32: every group's sum times its weight -- weights is (8,), one factor per group, or (8, 3), one per group and
    channel -- the products added from the left, the total divided by n: (((w0 g0) + (w1 g1)) + ... + (w7 g7)) / n, every product, add and the
    division one fp32 operation; 0 where n == 0.  With weights of 1 that is lights_sum(rec) / n."""
    rec = _lights_records(rec)
    w = np.asarray(weights, np.float32)
    if w.shape not in ((abi.LIGHTS_GROUPS,), (abi.LIGHTS_GROUPS, 3)):
        raise ValueError("lights_mix(): weights must have the shape (8,) or (8, 3)")
    w = np.broadcast_to(w.reshape(abi.LIGHTS_GROUPS, -1), (abi.LIGHTS_GROUPS, 3))
    sums = rec["group"]["sum"].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        out = w[0] * sums[..., 0, :]
        for g in range(1, abi.LIGHTS_GROUPS):
            out = out + w[g] * sums[..., g, :]
    return _bounces_per_sample(rec, out)


# ---- OpenEXR pass layers (include/rene_hip.h: rene_output_exr_passes) ------------------------------------------------------------------------------
EXR_PASS_LAYERS = {"ao": abi.EXRP_AO, "bent": abi.EXRP_BENT, "bounces": abi.EXRP_BOUNCES, "direct": abi.EXRP_DIRECT, "indirect": abi.EXRP_INDIRECT,
                   "lights": abi.EXRP_LIGHTS, "length": abi.EXRP_LENGTH}
# which pass's records a layer reads: the keys of `sources`
EXR_PASS_SOURCES = {"occlusion": abi.EXRP_AO | abi.EXRP_BENT, "direct": abi.EXRP_DIRECT | abi.EXRP_INDIRECT, "bounces": abi.EXRP_BOUNCES | abi.EXRP_LENGTH,
                    "lights": abi.EXRP_LIGHTS}
_EXR_PASS_ALL = ("ao", "bent", "bounces", "direct", "indirect", "lights", "length")


def exr_passes_mask(layers) -> int:
    """The RENE_EXRP_* mask of layer names ("ao", "bent", "direct", "indirect", "bounces", "length", "lights"), or the mask itself."""
    if isinstance(layers, int):
        return layers
    if isinstance(layers, str):
        layers = (layers,)
    mask = 0
    for name in layers:
        if name not in EXR_PASS_LAYERS:
            raise ValueError(f"layers must be among {sorted(EXR_PASS_LAYERS)}, not {name!r}")
        mask |= EXR_PASS_LAYERS[name]
    return mask


def _exr_passes_groups(groups) -> int:
    """An 8-bit mask of light groups from the mask itself, None (0: all eight) or the groups' numbers."""
    if groups is None:
        return 0
    if isinstance(groups, int):
        return groups
    mask = 0
    for g in groups:
        mask |= 1 << _lights_group("exr_passes", g)
    return mask


def _exr_passes_params(layers, groups, group_names, sources=None):
    """abi.ExrPassesParams of the arguments, and what it points at.  group_names: None, a list of up to eight names (None: no name) or {group: name};
    sources: {pass name: address}."""
    p = abi.ExrPassesParams()
    lib().rene_exr_passes_params_default(C.byref(p))
    p.layers, p.groups = exr_passes_mask(layers), _exr_passes_groups(groups)
    keep = []
    if group_names is not None:
        names = [None] * abi.LIGHTS_GROUPS
        for g, name in (group_names.items() if isinstance(group_names, dict) else enumerate(group_names)):
            names[_lights_group("exr_passes", g)] = None if name is None else (name.encode() if isinstance(name, str) else bytes(name))
        if any(n is not None and b"\0" in n for n in names):
            raise ValueError("a name holds a 0 byte")
        arr = (C.c_char_p * abi.LIGHTS_GROUPS)(*names)
        keep += [arr, names]
        p.group_names = arr
    for name, address in (sources or {}).items():
        if name not in EXR_PASS_SOURCES:
            raise ValueError(f"sources must be among {sorted(EXR_PASS_SOURCES)}, not {name!r}")
        setattr(p, name, address)
    return p, keep


def exr_passes_layout(xres: int, yres: int, layers=_EXR_PASS_ALL, groups=None, group_names=None) -> tuple[int, int, int]:
    """rene_exr_passes_layout: (attribute bytes, body bytes, bytes per pixel) of an xres x yres file of the pass `layers`, the light `groups` (a mask,
    a list of group numbers, None: all eight) and their names (host only).  The uncompressed file is attributes + 8 * yres of table + body."""
    p, keep = _exr_passes_params(layers, groups, group_names)
    head, body, bpp = C.c_size_t(), C.c_size_t(), C.c_uint32()
    _check(lib().rene_exr_passes_layout(xres, yres, C.byref(p), C.byref(head), C.byref(body), C.byref(bpp)))
    return head.value, body.value, bpp.value


def exr_passes_attributes(xres: int, yres: int, layers=_EXR_PASS_ALL, groups=None, group_names=None, compression="none") -> bytes:
    """rene_exr_passes_attributes: the file from the magic through the header's terminating 0 -- the channel list, the eight attributes of every
    file of this library's and, where a chosen light group has a name, rene/lightGroups (host only)."""
    p, keep = _exr_passes_params(layers, groups, group_names)
    n = exr_passes_layout(xres, yres, layers, groups, group_names)[0]
    buf = C.create_string_buffer(n)
    _check(lib().rene_exr_passes_attributes(xres, yres, C.byref(p), exr_compression(compression), buf, n))
    return buf.raw


def exr_passes_table(xres: int, yres: int, attributes_bytes: int, bytes_per_pixel: int) -> bytes:
    """The offset table of an uncompressed file: yres uint64, chunk y at attributes + 8 * yres + y * (8 + xres * bytes_per_pixel)."""
    return (attributes_bytes + 8 * yres + np.arange(yres, dtype=np.uint64) * np.uint64(8 + xres * bytes_per_pixel)).astype("<u8").tobytes()


def exr_passes_body_host(xres: int, yres: int, layers=_EXR_PASS_ALL, groups=None, *, occlusion=None, direct=None, bounces=None, lights=None,
                         beauty_sum=None) -> bytes:
    """rene_exr_passes_body_host: the body packed on the host from (yres, xres) record arrays of the passes the layers read (abi.OCCLUSION_DTYPE,
    DIRECT_DTYPE, BOUNCES_DTYPE, LIGHTS_DTYPE) and, for "indirect", beauty_sum, (yres, xres, 3) or (yres, xres, 4) float32 sums: the definition
    the device is held to."""
    keep, sources = [], {}
    for name, rec, records in (("occlusion", occlusion, _occlusion_records), ("direct", direct, _direct_records), ("bounces", bounces, _bounces_records),
                               ("lights", lights, _lights_records)):
        if rec is None:
            continue
        rec = np.ascontiguousarray(records(rec))
        if rec.shape != (yres, xres):
            raise ValueError(f"exr_passes_body_host(): the {name} records have the shape {rec.shape}, the film {(yres, xres)}")
        keep.append(rec)
        sources[name] = rec.ctypes.data
    p, keep2 = _exr_passes_params(layers, groups, None, sources)
    beauty = None
    if beauty_sum is not None:
        beauty = np.ascontiguousarray(np.asarray(beauty_sum, np.float32)[..., :3])
        if beauty.shape != (yres, xres, 3):
            raise ValueError("exr_passes_body_host(): beauty_sum must be (yres, xres, 3) or (yres, xres, 4)")
    body = exr_passes_layout(xres, yres, layers, groups)[1]
    buf = C.create_string_buffer(body)
    _check(lib().rene_exr_passes_body_host(xres, yres, C.byref(p), None if beauty is None else beauty.ctypes.data_as(C.c_void_p), buf, body))
    return buf.raw


def _exr_passes_sources(self, sources) -> dict:
    """{pass name: device address} of `sources`, {pass name: a uint8 torch tensor of that pass's records on the context's device}."""
    sizes = {"occlusion": occlusion_bytes, "direct": direct_bytes, "bounces": bounces_bytes, "lights": lights_bytes}
    out = {}
    for name, tensor in (sources or {}).items():
        if name not in sizes:
            raise ValueError(f"sources must be among {sorted(sizes)}, not {name!r}")
        _check_tensor("exr_passes", tensor, self.device, ("uint8",), numel=sizes[name](self.xres, self.yres))
        out[name] = tensor.data_ptr()
    return out


def _exr_passes_into(self, tensor, layers=_EXR_PASS_ALL, groups=None, group_names=None, sources=None):
    """rene_output_exr_passes into a caller-owned torch tensor on the context's device: contiguous, uint8, of the body's size (exr_passes_layout).
    Only the bytes of the tiles this context owns are written, and the prefix of their rows, so the tile shards of one device fill one tensor
    between them; the file is exr_passes_attributes() + exr_passes_table() + the tensor's bytes, or the attributes + exr_compress_rows() of the
    tensor.  sources: {"occlusion" | "direct" | "bounces" | "lights": a uint8 tensor of that pass's records (occlusion_into's and the like)};
    a pass without one is read from the library-owned result of its last call.  Returns the tensor."""
    p, keep = _exr_passes_params(layers, groups, group_names, _exr_passes_sources(self, sources))
    _check_tensor("exr_passes_into", tensor, self.device, ("uint8",), what="body")
    _check(lib().rene_output_exr_passes(self._h, C.byref(p), C.c_void_p(tensor.data_ptr()), tensor.numel()))
    return tensor


def _exr_passes(self, path=None, layers=_EXR_PASS_ALL, groups=None, group_names=None, compression="none", sources=None) -> bytes:
    """The pass layers as a scan-line OpenEXR file of HALF channels, packed on the device (rene_output_exr_passes): "ao" and "bent" from the last
    occlusion(), "direct" and "indirect" from the last direct() (indirect: beauty - direct, so the context must hold exactly the pass's frames),
    "bounces" (depth0 .. depth9) and "length" (pathlength) from the last bounces(), "lights" (light0 .. light7, or the groups of `groups`, named
    by group_names in the rene/lightGroups attribute) from the last lights() -- or from the record tensors of `sources`.  compression: "none" or
    "zips".  Only the file's bytes cross PCIe.  Returns them; written to `path` too (through path + ".tmp") where one is given."""
    code = exr_compression(compression)
    if self._shard_count > 1:
        raise ReneError(-4, "exr_passes(): a row spans tiles of several shards; fill one body with exr_passes_into() and compress it with exr_compress_rows()")
    p, keep = _exr_passes_params(layers, groups, group_names, _exr_passes_sources(self, sources))
    _check(lib().rene_output_exr_passes(self._h, C.byref(p), None, 0))
    attributes = exr_passes_attributes(self.xres, self.yres, layers, groups, group_names, code)
    body_ptr, body_bytes = _result_buffer(self, lib().rene_exr_passes_buffer)
    row_bytes = body_bytes // self.yres - 8
    if code == abi.EXR_COMPRESSION_NONE:
        body = _download_result(self, lib().rene_download_exr_passes, (body_bytes,), np.uint8)
        data = attributes + exr_passes_table(self.xres, self.yres, len(attributes), row_bytes // self.xres) + body.tobytes()
    else:
        written = C.c_size_t()
        _check(lib().rene_exr_compress_rows(self._h, row_bytes, self.yres, len(attributes), code, C.c_void_p(body_ptr), body_bytes, None, 0, C.byref(written)))
        data = attributes + _download_exr_tail(self)
    if path is not None:
        tmp = str(path) + ".tmp"
        with open(tmp, "wb") as f:
            f.write(data)
        os.replace(tmp, path)
    return data


def _exr_passes_buffer(self):
    """rene_exr_passes_buffer: (device pointer, bytes) of the last body packed into the library's own buffer."""
    return _result_buffer(self, lib().rene_exr_passes_buffer)


Renderer.exr_passes = _exr_passes
Renderer.exr_passes_into = _exr_passes_into
Renderer.exr_passes_buffer = _exr_passes_buffer


def output_thresholds() -> np.ndarray:
    """rene_output_thresholds: the 255 thresholds of the device's sRGB transform -- T[k] is the smallest float to_rgb8(., 1) maps to k + 1 (host only)."""
    out = np.empty(255, np.float32)
    lib().rene_output_thresholds(out.ctypes.data_as(C.c_void_p))
    return out


def output_probe(values, transform: str = "srgb", device: int = 0) -> np.ndarray:
    """rene_output_probe: the bytes of the means `values` under "srgb", "aov" or "aov_normal", computed on the device by the function the
    kernel of rgb8() uses; an array of values' shape."""
    if transform not in _OUTPUT_TRANSFORMS:
        raise ValueError(f"transform must be one of {sorted(_OUTPUT_TRANSFORMS)}, not {transform!r}")
    v = np.ascontiguousarray(values, dtype=np.float32)
    out = np.empty(v.shape, np.uint8)
    _check(lib().rene_output_probe(device, _OUTPUT_TRANSFORMS[transform], v.size, v.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


# ---- tone-mapped output and the luminance histogram (include/rene_hip.h: rene_output_tonemapped, rene_luminance_histogram) ------------------------
_TONEMAPS = {"clamp": abi.TONEMAP_CLAMP, "reinhard": abi.TONEMAP_REINHARD, "aces": abi.TONEMAP_ACES}


def _tonemap_op(tonemap) -> int:
    if tonemap not in _TONEMAPS:
        raise ValueError(f"tonemap must be one of {sorted(_TONEMAPS)}, not {tonemap!r}")
    return _TONEMAPS[tonemap]


def tonemap_params_default() -> abi.TonemapParams:
    """rene_tonemap_params_default: RADIANCE, RGB8, CLAMP, scale 1, white 4 (host only)."""
    p = abi.TonemapParams()
    lib().rene_tonemap_params_default(C.byref(p))
    return p


def exposure_e8(ev) -> int:
    """An exposure in EV as eighth-stops: the nearest, halves upward."""
    return int(np.floor(float(ev) * 8.0 + 0.5))


def exposure_scale(e8: int) -> np.float32:
    """rene_exposure_scale: the fp32 factor 2^(e8 / 8) of an exposure in eighth-stops, from eight literals and ldexpf (host only)."""
    return np.float32(lib().rene_exposure_scale(int(e8)))


def _tonemap_params(r, source, alpha, tonemap, exposure, white, key):
    """The rene_tonemap_params of rgb8()'s keywords, or None where none of them is given (the call is then rene_output_8bit, as it always was)."""
    if tonemap is None and exposure is None and white is None and key is None:
        return None
    p = tonemap_params_default()
    p.source, p.format = _output_params(source, alpha).source, abi.OUTPUT_RGBA8 if alpha else abi.OUTPUT_RGB8
    p.op = _tonemap_op("clamp" if tonemap is None else tonemap)
    if white is not None:
        p.white = float(white)
    if isinstance(exposure, str):
        if exposure != "auto":
            raise ValueError(f"exposure must be a number of EV or \"auto\", not {exposure!r}")
        e8 = auto_exposure_e8(r.luminance_stats(source), abi.EXPOSURE_KEY_E8 if key is None else key)
    else:
        e8 = 0 if exposure is None else exposure_e8(exposure)
    p.scale = exposure_scale(e8)
    return p


def _luminance_stats(self, source: str = "radiance") -> abi.LuminanceStats:
    """rene_luminance_histogram: the luminance histogram of `source` ("radiance", "denoised", "denoised_mean", "robust") over the pixels this
    context owns, counted on the device -- .counts[256], .n_dark, .n_pixels."""
    out = abi.LuminanceStats()
    _check(lib().rene_luminance_histogram(self._h, _output_params(source, False).source, C.byref(out)))
    return out


Renderer.luminance_stats = _luminance_stats


def luminance_counts(stats: abi.LuminanceStats) -> np.ndarray:
    """The 256 counts of a histogram as a uint32 array."""
    return np.array(stats.counts, dtype=np.uint32)


def luminance_combine(parts) -> abi.LuminanceStats:
    """rene_luminance_combine: the element-wise sum of the histograms of one image's tile shards (host only)."""
    parts = list(parts)
    arr = (abi.LuminanceStats * len(parts))(*parts)
    out = abi.LuminanceStats()
    _check(lib().rene_luminance_combine(arr, len(parts), C.byref(out)))
    return out


def luminance_mean_bin_x256(stats: abi.LuminanceStats) -> int:
    return int(lib().rene_luminance_mean_bin_x256(C.byref(stats)))


def luminance_percentile_bin(stats: abi.LuminanceStats, per_mille: int) -> int:
    return int(lib().rene_luminance_percentile_bin(C.byref(stats), per_mille))


def auto_exposure_e8(stats: abi.LuminanceStats, key: int = abi.EXPOSURE_KEY_E8) -> int:
    """rene_auto_exposure_e8: the exposure, in eighth-stops, that moves the histogram's mean log2 luminance onto key / 8 (host only, integers)."""
    return int(lib().rene_auto_exposure_e8(C.byref(stats), int(key)))


def _means(means):
    a = np.ascontiguousarray(means, dtype=np.float32)
    if a.ndim < 1 or a.shape[-1] not in (3, 4):
        raise ValueError(f"means must be [..., 3] or [..., 4], not {a.shape}")
    return a


def tonemap_rgb8(means, tonemap: str = "clamp", scale=1.0, white=4.0) -> np.ndarray:
    """rene_tonemap_rgb8: the host form of rgb8(tonemap=...) -- [..., 3 or 4] fp32 means to [..., 3] bytes under the factor `scale` (host only)."""
    a = _means(means)
    out = np.empty(a.shape[:-1] + (3,), np.uint8)
    _check(lib().rene_tonemap_rgb8(a.ctypes.data_as(C.c_void_p), a.size // a.shape[-1], a.shape[-1], _tonemap_op(tonemap), float(scale), float(white), out.ctypes.data_as(C.c_void_p)))
    return out


def luminance_histogram_host(means) -> abi.LuminanceStats:
    """rene_luminance_histogram_host: the host form of Renderer.luminance_stats on [..., 3 or 4] fp32 means (host only)."""
    a = _means(means)
    out = abi.LuminanceStats()
    _check(lib().rene_luminance_histogram_host(a.ctypes.data_as(C.c_void_p), a.size // a.shape[-1], a.shape[-1], C.byref(out)))
    return out


def tonemap_probe(rgb, tonemap: str = "clamp", scale=1.0, white=4.0, device: int = 0) -> np.ndarray:
    """rene_tonemap_probe: the bytes of the [..., 3] means `rgb`, computed on the device by the per-pixel function the kernel of rgb8(tonemap=...)
    uses; an array of rgb's shape."""
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    if a.ndim < 1 or a.shape[-1] != 3:
        raise ValueError(f"rgb must be [..., 3], not {a.shape}")
    out = np.empty(a.shape, np.uint8)
    _check(lib().rene_tonemap_probe(device, _tonemap_op(tonemap), float(scale), float(white), a.size // 3, a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def _emitter_pdf(self, origins, directions) -> np.ndarray:
    """Device emitter-pdf probe (lib.rs:301-318 + 959-1066): pdf_l of each ray against the emitter-only structure."""
    o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(o.shape[0], np.float32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    _check(lib().rene_emitter_pdf(self._h, o.shape[0], p(o), p(d), p(out)))
    return out


Renderer.emitter_pdf = _emitter_pdf


def _emitter_pdf_form(self, form: int, origins, directions) -> np.ndarray:
    """rene_emitter_pdf_form: form 0 is emitter_pdf; 1 and 2 are the small-scene kernels' LDS forms (2: direction normalised first)."""
    o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(o.shape[0], np.float32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    _check(lib().rene_emitter_pdf_form(self._h, int(form), o.shape[0], p(o), p(d), p(out)))
    return out


def _emit_sample(self, form: int, seeds) -> np.ndarray:
    """rene_emit_sample: (n, 8) float32 -- the emitter point of PCG32si::new(seed), the bits of the object and of the stream's next u32
    (view columns 3 and 4 as uint32), zeros.  form 0: the global tables; form 1: the LDS image of a small scene."""
    s = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
    out = np.zeros((s.shape[0], 8), np.float32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    _check(lib().rene_emit_sample(self._h, int(form), s.shape[0], p(s), p(out)))
    return out


Renderer.emitter_pdf_form = _emitter_pdf_form
Renderer.emit_sample = _emit_sample


def _frame_stream_probe(self, first_frame: int, n_frames: int) -> np.ndarray:
    """rene_frame_stream_probe: the frame-stream table of global frames first_frame .. first_frame + n_frames - 1 as the fill kernel writes it,
    (n_frames, 50, 4) float32 -- on_light.xyz, and the roulette number with the coin's decision in its sign bit (include/rene_hip.h)."""
    out = np.zeros((n_frames, abi.FRAME_STREAM_DEPTHS, 4), np.float32)
    _check(lib().rene_frame_stream_probe(self._h, first_frame, n_frames, out.ctypes.data_as(C.c_void_p)))
    return out


Renderer.frame_stream_probe = _frame_stream_probe


def _load_chains(self, chains, first_frame: int = 0, n_frames: int | None = None, tile_frames=None):
    """rene_load_chains (a probe for tests of the chain passes): put `chains`, an (8, 3, yres, xres, 3) float32 array -- chain, layer (radiance,
    normal, albedo), rows top first -- into a fresh or reset context as if render(first_frame, n_frames) had left them, bit for bit.  n_frames
    defaults to 8 (one frame per chain), under tile_frames to their largest; `tile_frames`, a (tiles_y, tiles_x) array, gives every tile its own frame count (each <= n_frames, one equal to it: the state
    an adaptive job leaves).  Every reading call then works as after a render; render() and set_active_tiles() are refused until reset()."""
    c = np.asarray(chains)
    if c.dtype != np.float32 or c.shape != (8, 3, self.yres, self.xres, 3):
        raise ValueError(f"load_chains: expected a float32 array of shape {(8, 3, self.yres, self.xres, 3)}, got {c.dtype} {c.shape}")
    c = np.ascontiguousarray(c)
    tf, n_tiles = None, 0
    if tile_frames is not None:
        tf = np.ascontiguousarray(tile_frames, dtype=np.uint32)
        if tf.shape != _tile_grid(self):
            raise ValueError(f"load_chains: tile_frames must be a {_tile_grid(self)} array, got {tf.shape}")
        n_tiles = tf.size
    if n_frames is None:
        n_frames = 8 if tf is None else int(tf.max(initial=0))
    _check(lib().rene_load_chains(self._h, c.ctypes.data_as(C.c_void_p), c.size, first_frame, n_frames,
                                  None if tf is None else tf.ctypes.data_as(C.c_void_p), n_tiles))


Renderer.load_chains = _load_chains


# ---- checkpoint: save, restore and resume a job (include/rene_hip.h) ----

def _state_params(chunk_tiles):
    if chunk_tiles is None:
        return None
    p = abi.StateParams()
    lib().rene_state_params_default(C.byref(p))
    p.chunk_tiles = int(chunk_tiles)
    return C.byref(p)


def _state_blob(blob) -> np.ndarray:
    b = np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else np.asarray(blob)
    if b.dtype != np.uint8 or b.ndim != 1:
        raise ValueError("a state part is a one-dimensional uint8 array (or bytes)")
    return np.ascontiguousarray(b)


def state_bytes(xres: int, yres: int, shard_rank: int = 0, shard_count: int = 1) -> int:
    """rene_state_bytes: the bytes of the part a context of tile shard `shard_rank` of `shard_count` saves for an xres x yres film (host only)."""
    return int(lib().rene_state_bytes(xres, yres, shard_rank, shard_count))


def scene_fingerprint(scene) -> tuple[int, int]:
    """rene_scene_fingerprint: 128 bits over the scene's tables as rene_create receives them (host only)."""
    packed = scene if hasattr(scene, "byref") else scene.to_desc()
    out = (C.c_uint64 * 2)()
    _check(lib().rene_scene_fingerprint(packed.byref(), out))
    return int(out[0]), int(out[1])


def state_info(blob) -> abi.StateInfo:
    """rene_state_inspect: a part's header, after the whole part has been checked for consistency (host only)."""
    b = _state_blob(blob)
    info = abi.StateInfo()
    info.struct_size = C.sizeof(abi.StateInfo)
    _check(lib().rene_state_inspect(b.ctypes.data_as(C.c_void_p), b.size, C.byref(info)))
    return info


def state_tiles(blob) -> np.ndarray:
    """rene_state_tiles: a part's tile table as a structured array (abi.STATE_TILE_DTYPE), in table order (host only)."""
    b = _state_blob(blob)
    out = np.zeros(state_info(b).n_tiles, dtype=abi.STATE_TILE_DTYPE)
    _check(lib().rene_state_tiles(b.ctypes.data_as(C.c_void_p), b.size, out.ctypes.data_as(C.c_void_p), out.size))
    return out


def state_file_info(path):
    """rene_state_inspect_file: (header info, tile table) of a part in a file, of which only header and table are read (host only)."""
    info = abi.StateInfo()
    info.struct_size = C.sizeof(abi.StateInfo)
    _check(lib().rene_state_inspect_file(os.fsencode(path), C.byref(info), None, 0))
    tiles = np.zeros(info.n_tiles, dtype=abi.STATE_TILE_DTYPE)
    _check(lib().rene_state_inspect_file(os.fsencode(path), C.byref(info), tiles.ctypes.data_as(C.c_void_p), tiles.size))
    return info, tiles


def state_verify(blob) -> None:
    """rene_state_verify: every tile's checksum recomputed from its payload; raises ReneError naming the first tile that differs (host only)."""
    b = _state_blob(blob)
    _check(lib().rene_state_verify(b.ctypes.data_as(C.c_void_p), b.size))


def _shard(self) -> tuple[int, int]:
    return (self._shard_rank, self._shard_count) if self._shard_mode == abi.SHARD_TILES and self._shard_count > 1 else (0, 1)


def _save_state(self, chunk_tiles: int | None = None, out: np.ndarray | None = None) -> np.ndarray:
    """rene_save_state: the context's state -- the eight frame chains of the tiles it owns and the bookkeeping -- as a uint8 array (`out`, where
    given: a uint8 array of at least that size, say the numpy view of a pinned tensor, which the device then writes without a staging)."""
    need = state_bytes(self.xres, self.yres, *_shard(self))
    buf = np.empty(need, np.uint8) if out is None else out
    if buf.dtype != np.uint8 or buf.ndim != 1 or not buf.flags.c_contiguous:
        raise ValueError("save_state: out must be a contiguous one-dimensional uint8 array")
    written = C.c_size_t()
    _check(lib().rene_save_state(self._h, _state_params(chunk_tiles), buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(written)))
    return buf[:written.value]


def _restore_state(self, *parts, chunk_tiles: int | None = None):
    """rene_restore_state: put one or more saved parts into this fresh (or reset) context; rendering then goes on at frame F + N, bit for bit as
    the job that was saved would have."""
    blobs = [_state_blob(p) for p in parts]
    ptrs = (C.c_void_p * len(blobs))(*[b.ctypes.data for b in blobs])
    sizes = (C.c_size_t * len(blobs))(*[b.size for b in blobs])
    _check(lib().rene_restore_state(self._h, _state_params(chunk_tiles), ptrs, sizes, len(blobs)))


def _save_state_file(self, path, chunk_tiles: int | None = None):
    """rene_save_state_file: save_state streamed to `path` (written as path + ".tmp", then renamed: the file is whole or absent)."""
    _check(lib().rene_save_state_file(self._h, _state_params(chunk_tiles), os.fsencode(path)))


def _restore_state_files(self, *paths, chunk_tiles: int | None = None):
    """rene_restore_state_files: restore_state streamed from the parts' files."""
    arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
    _check(lib().rene_restore_state_files(self._h, _state_params(chunk_tiles), arr, len(paths)))


Renderer.save_state = _save_state
Renderer.restore_state = _restore_state
Renderer.save_state_file = _save_state_file
Renderer.restore_state_files = _restore_state_files


def _ray_dump(self, first_frame: int, n_frames: int, capacity: int):
    """(rays [n][8] f32 -- o.xyz, tmax, d.xyz, meta bits --, queries issued) of the frames rendered: rene_ray_dump (the J1 gate's input)."""
    out = np.zeros((capacity, 8), np.float32)
    n = C.c_uint64()
    _check(lib().rene_ray_dump(self._h, first_frame, n_frames, capacity, out.ctypes.data_as(C.c_void_p), C.byref(n)))
    return out[:min(capacity, n.value)], n.value


def _trace_queue(self, o_tmax, d_flags, fp16: bool, refill_min: int = 16, leaf_min: int = 6, blocks_per_cu: int = 0, repeats: int = 3,
                 want_hits: bool = False, want_steps: bool = True):
    """rene_trace_queue: (milliseconds of the fastest launch, hits [n][4] or None, steps5 or None)."""
    o = np.ascontiguousarray(o_tmax, np.float32)
    d = np.ascontiguousarray(d_flags)
    n = o.shape[0]
    hits = np.zeros((n, 4), np.float32) if want_hits else None
    steps = np.zeros(5, np.uint64) if want_steps else None
    ms = C.c_float()
    p = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
    _check(lib().rene_trace_queue(self._h, n, p(o), p(d), int(fp16), refill_min, leaf_min, blocks_per_cu, repeats, p(hits), C.byref(ms), p(steps)))
    return ms.value, hits, steps


Renderer.ray_dump = _ray_dump
Renderer.trace_queue = _trace_queue


def _comm_init(self, n_ranks: int, rank: int, unique_id: bytes):
    """Join an RCCL communicator (one context per GPU); `unique_id` = comm_unique_id() of rank 0, handed over by the host."""
    buf = (C.c_uint8 * abi.COMM_ID_BYTES).from_buffer_copy(unique_id)
    _check(lib().rene_comm_init(self._h, n_ranks, rank, buf))


def _reduce(self, root: int = 0):
    _check(lib().rene_reduce(self._h, root))


def _gather_tiles(self, root: int = 0):
    _check(lib().rene_gather_tiles(self._h, root))


Renderer.comm_init = _comm_init
Renderer.reduce = _reduce
Renderer.gather_tiles = _gather_tiles


def comm_unique_id() -> bytes:
    buf = (C.c_uint8 * abi.COMM_ID_BYTES)()
    _check(lib().rene_comm_unique_id(buf))
    return bytes(buf)


def pcg_probe(seed: int, n: int, device: int = 0) -> np.ndarray:
    """n outputs of PCG32si::new(seed) computed on the device (rene_pcg_probe)."""
    out = np.zeros(n, np.uint32)
    _check(lib().rene_pcg_probe(device, seed & 0xFFFFFFFF, n, out.ctypes.data_as(C.c_void_p)))
    return out


def _bsdf_eval(self, material_index: int, normals, uvs, wo, wi, seeds) -> np.ndarray:
    """Device BSDF probe: returns (n, 12) = f.rgb, pdf, s_wi.xyz, s_f.rgb, s_pdf, lobe count."""
    a = [np.ascontiguousarray(v, dtype=np.float32) for v in (normals, uvs, wo, wi)]
    sd = np.ascontiguousarray(seeds, dtype=np.uint32)
    n = sd.size
    out = np.zeros((n, 12), np.float32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    _check(lib().rene_bsdf_eval(self._h, material_index, n, p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(sd), p(out)))
    return out


Renderer.bsdf_eval = _bsdf_eval


def _medium_eval(self, medium_index: int, rd, t_max, wo, wi, seeds) -> np.ndarray:
    """Device medium probe (volpath scenes): (n, 16), layout of rene_medium_eval in include/rene_hip.h."""
    a = [np.ascontiguousarray(v, dtype=np.float32) for v in (rd, t_max, wo, wi)]
    sd = np.ascontiguousarray(seeds, dtype=np.uint32)
    out = np.zeros((sd.size, 16), np.float32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    _check(lib().rene_medium_eval(self._h, medium_index, sd.size, p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(sd), p(out)))
    return out


Renderer.medium_eval = _medium_eval


def _transmittance(self, emit: bool, medium_index: int, origins, directions) -> np.ndarray:
    """Device probe of the transmittance walks (volpath scenes): (n, 4), layout of rene_transmittance in include/rene_hip.h."""
    o, d = (np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3) for v in (origins, directions))
    if o.shape != d.shape:
        raise ValueError("origins and directions differ in shape")
    out = np.zeros((len(o), 4), np.float32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    _check(lib().rene_transmittance(self._h, int(bool(emit)), medium_index, len(o), p(o), p(d), p(out)))
    return out


Renderer.transmittance = _transmittance


def pack_info(scene) -> abi.PackInfo:
    """Host-only validation + flattening + BVH build (no GPU needed)."""
    packed = scene if hasattr(scene, "byref") else scene.to_desc()
    info = abi.PackInfo()
    _check(lib().rene_scene_pack_info(packed.byref(), C.byref(info)))
    return info


def small_items(scene, which: int = 0):
    """rene_scene_small_items: (records, n_loop) -- the item list of the small-scene kernels as a (n, 16) uint32 array of the records' words
    (loop items first, box auxiliary records behind them) and the number of loop items; `which` 0 = main structure, 1 = emitter structure.
    Host only.  Word 15, bit 31 (abi.SMALL_ITEM_EMIT_TWIN): the main item that also answers the emitter query."""
    packed = scene if hasattr(scene, "byref") else scene.to_desc()
    n_loop, n_total = C.c_uint32(0), C.c_uint32(0)
    _check(lib().rene_scene_small_items(packed.byref(), which, None, 0, C.byref(n_loop), C.byref(n_total)))
    out = np.zeros((n_total.value, 16), np.uint32)
    if n_total.value:
        _check(lib().rene_scene_small_items(packed.byref(), which, out.ctypes.data_as(C.c_void_p), n_total.value, C.byref(n_loop), None))
    return out, n_loop.value


def plan_memory(scene, seed: int = abi.DEFAULT_SEED, device: int = 0, flags: int = 0, shard_mode: int = abi.SHARD_TILES,
                shard_rank: int = 0, shard_count: int = 1, framebuffer_ptr: int | None = None, stream_ptr: int | None = None) -> dict:
    """The device memory a Renderer of this scene and these options would allocate, in bytes (no GPU needed): chain_bytes,
    version_bytes, image_bytes, scene_bytes, queue_bytes, total_bytes.  Raises ReneError where Renderer() would refuse."""
    packed = scene if hasattr(scene, "byref") else scene.to_desc()
    o = abi.Opts()
    o.struct_size = C.sizeof(abi.Opts)
    o.seed, o.device, o.flags = seed & 0xFFFFFFFF, device, flags
    o.shard_mode, o.shard_rank, o.shard_count = shard_mode, shard_rank, shard_count
    o.framebuffer = framebuffer_ptr
    o.stream = stream_ptr
    plan = abi.MemoryPlan()
    _check(lib().rene_plan_memory(packed.byref(), C.byref(o), C.byref(plan)))
    return plan.as_dict()


def to_rgb8(sums: np.ndarray, n_samples: int) -> np.ndarray:
    """average + gamma + quantise (rene/src/main.rs:1758-1792)."""
    a = np.ascontiguousarray(sums, dtype=np.float32)
    out = np.empty(a.shape, dtype=np.uint8)
    lib().rene_to_rgb8(a.ctypes.data_as(C.c_void_p), a.size, n_samples, out.ctypes.data_as(C.c_void_p))
    return out


def to_aov8(sums: np.ndarray, n_samples: int, is_normal: bool) -> np.ndarray:
    a = np.ascontiguousarray(sums, dtype=np.float32)
    out = np.empty(a.shape, dtype=np.uint8)
    lib().rene_to_aov8(a.ctypes.data_as(C.c_void_p), a.size, n_samples, int(is_normal), out.ctypes.data_as(C.c_void_p))
    return out


def frame_seeds(master_seed: int, first_frame: int, n: int) -> np.ndarray:
    out = np.empty(n, dtype=np.uint32)
    lib().rene_frame_seeds(master_seed & 0xFFFFFFFF, first_frame, n, out.ctypes.data_as(C.c_void_p))
    return out
