"""CPU: the denoiser hand-off's host surface (rene_export_features: the struct, the defaults, the pure host functions, argument checks, the command
line) and its specification -- the numpy restatement of tests/features_reference.py on the CPU oracle's chains: do the two half-images add up to
the image, is the variance one, and what is the fp32 rounding of its tile sums (the figure tests/test_gpu_features.py takes its bound from)?"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import features_reference as fr
from atrous_reference import chains_of
from conftest import ROOT
from rene_amd import abi, api, scenes

THREADS = 8
CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
NEW_SYMBOLS = ("rene_feature_params_default", "rene_feature_channels", "rene_export_features", "rene_features_buffer", "rene_download_features")

def test_struct_and_constants_match_the_header():
    fields = ("struct_size", "features", "format", "layout")
    names = ("COLOR", "ALBEDO", "NORMAL", "VARIANCE", "HALF_A", "HALF_B", "FRAMES")
    prog = '#include <stdio.h>\n#include "rene_hip.h"\nint main(void){\n'
    prog += 'printf("%zu\\n", sizeof(rene_feature_params));\n'
    for f in fields:
        prog += f'printf("%zu\\n", offsetof(rene_feature_params, {f}));\n'
    for n in names:
        prog += f'printf("%u\\n", (unsigned)RENE_FEATURE_{n});\n'
    prog += 'printf("%d %d %d %d\\n", RENE_FEATURES_F32, RENE_FEATURES_F16, RENE_FEATURES_CHW, RENE_FEATURES_HWC);\nprintf("%u\\n", RENE_ABI_VERSION);\nreturn 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = list(map(int, subprocess.check_output([exe]).split()))
    assert out[0] == C.sizeof(abi.FeatureParams) == 16
    assert out[1:5] == [getattr(abi.FeatureParams, f).offset for f in fields] == [0, 4, 8, 12]
    assert out[5:12] == [getattr(abi, "FEATURE_" + n) for n in names] == [getattr(fr, n) for n in names] == [1 << b for b in range(7)]
    assert out[12:16] == [abi.FEATURES_F32, abi.FEATURES_F16, abi.FEATURES_CHW, abi.FEATURES_HWC] == [0, 1, 0, 1]
    assert out[16] == abi.ABI_VERSION == 7  # new symbols and a struct_size-carrying struct break no caller
    assert abi.FEATURE_ALL == fr.ALL == 127 and abi.FEATURE_DEFAULT == fr.DEFAULT == 7
    for name in NEW_SYMBOLS:
        assert name in abi.EXPORTED_SYMBOLS


def test_feature_channels_for_every_mask(hip_lib):
    assert hip_lib.rene_feature_channels(0) == 0
    for mask in range(1, 128):
        want = sum(3 if bit in (0, 1, 2, 4, 5) else 1 for bit in range(7) if mask >> bit & 1)
        assert hip_lib.rene_feature_channels(mask) == api.feature_channels(mask) == fr.channels(mask) == want, mask
    assert hip_lib.rene_feature_channels(127) == 17 and hip_lib.rene_feature_channels(7) == 9
    for bad in (128, 129, 1 << 7 | 127, 1 << 31, 0xffffffff, 1 << 16 | 1):
        assert hip_lib.rene_feature_channels(bad) == 0 == fr.channels(bad), bad


def test_defaults_null_arguments_and_struct_size(hip_lib):
    p = api.feature_params_default()
    assert p.struct_size == C.sizeof(abi.FeatureParams) == 16
    assert p.features == abi.FEATURE_COLOR | abi.FEATURE_ALBEDO | abi.FEATURE_NORMAL and p.format == abi.FEATURES_F32 and p.layout == abi.FEATURES_HWC
    hip_lib.rene_feature_params_default(None)  # ignored
    assert hip_lib.rene_export_features(None, C.byref(p), None, 0) == -1 and b"NULL context" in hip_lib.rene_last_error()
    assert hip_lib.rene_export_features(None, None, None, 0) == -1
    ptr, n = C.c_void_p(), C.c_size_t()
    assert hip_lib.rene_features_buffer(None, C.byref(ptr), C.byref(n)) == -1 and hip_lib.rene_last_error()
    buf = (C.c_float * 4)()
    assert hip_lib.rene_download_features(None, buf, 16) == -1 and hip_lib.rene_last_error()
    assert hip_lib.rene_abi_version() == 7
    # the Python side refuses what it can before the library is asked
    for kw in (dict(dtype="bf16"), dict(layout="nchw")):
        with pytest.raises(ValueError):
            api._feature_params(abi.FEATURE_DEFAULT, **{"dtype": "f32", "layout": "hwc", **kw})


def test_cli_help_and_the_gpus_refusal(hip_lib):
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--features PREFIX" in r.stderr and ".pfm" in r.stderr
    r = subprocess.run([CLI, "scene.pbrt", "--features", "out", "--gpus", "2"], capture_output=True, text=True)
    assert r.returncode == 2 and "--features" in r.stderr and "--gpus 2" in r.stderr
    r = subprocess.run([CLI, "scene.pbrt", "--features"], capture_output=True, text=True)
    assert r.returncode == 2 and "needs a value" in r.stderr


# ---- closed forms on the restatement ------------------------------------------------------------------------------------------------
def _flat(means, n_c, h=3, w=5):
    """Chains whose means are means[c] in every channel and pixel (lum's weights add up to one: l_c = means[c])."""
    return np.stack([np.full((h, w, 3), float(n_c[c]) * means[c]) for c in range(8)])


def test_closed_forms():
    n_c = np.array([2, 1, 2, 1, 2, 1, 2, 1])
    means = [1.0, 3.0] * 4  # even chains 1, odd chains 3: N = 12, mean (8 + 12) / 12 = 5 / 3
    f = fr.features(_flat(means, n_c), n_c, dtype=np.float64)
    assert np.allclose(f[fr.COLOR], 5 / 3) and np.allclose(f[fr.HALF_A], 1.0) and np.allclose(f[fr.HALF_B], 3.0) and (f[fr.FRAMES] == 12).all()
    # v = sum (n_c / N) (l_c - l)^2 / (k - 1) = (8/12 (2/3)^2 + 4/12 (4/3)^2) / 7 = (8/27 + 16/27) / 7 = 8 / 63
    assert np.allclose(f[fr.VARIANCE], 8 / 63)
    assert (f[fr.ALBEDO] == 0).all() and (f[fr.NORMAL] == 0).all()  # no guide sums given
    g = fr.features(_flat(means, n_c), n_c, s_normal=np.full((3, 5, 3), 6.0), s_albedo=np.full((3, 5, 3), 3.0), dtype=np.float32)
    assert (g[fr.NORMAL] == 0.5).all() and (g[fr.ALBEDO] == 0.25).all() and g[fr.COLOR].dtype == np.float32
    # no frames: zeros everywhere, FRAMES included
    z = fr.features(np.ones((8, 2, 2, 3)), np.zeros(8, int))
    assert all(not v.any() for v in z.values()) and set(z) == {1, 2, 4, 8, 16, 32, 64}
    # the tensor: channels in bit order, both layouts
    t = fr.tensor(f, fr.ALL, "hwc")
    assert t.shape == (3, 5, 17) and np.allclose(t[0, 0], [5 / 3] * 3 + [0] * 6 + [8 / 63] + [1.0] * 3 + [3.0] * 3 + [12.0])
    assert np.array_equal(fr.tensor(f, fr.ALL, "chw"), np.moveaxis(t, -1, 0)) and fr.tensor(f, fr.VARIANCE | fr.FRAMES, "chw").shape == (2, 3, 5)
    assert fr.channel_slices(fr.COLOR | fr.VARIANCE | fr.HALF_B) == {fr.COLOR: slice(0, 3), fr.VARIANCE: slice(3, 4), fr.HALF_B: slice(4, 7)}
    # fp16: clamped, rounded to nearest even, subnormals kept, a NaN stays one
    x = np.array([1e6, -1e6, 65519.9, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -25, 3e-8 * 1.01, np.nan, np.inf], np.float32)
    h = fr.to_f16(x)
    assert h.dtype == np.float16 and h[:3].tolist() == [65504.0, -65504.0, 65504.0] and h[9] == 65504.0
    assert h[3] == 1.0 and h[4] == np.float16(1.0 + 2.0 ** -9)  # ties to even
    assert h[5] == 2.0 ** -24 and h[6] == 0 and h[7] == 2.0 ** -24 and np.isnan(h[8])


# ---- the specification on oracle renders ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell_frames(oracle_mod):
    """The twelve frames of cornell_box(40, 28) on the CPU oracle, once: [(radiance, normal, albedo sums of frame f)]."""
    o = oracle_mod.Oracle(scenes.cornell_box(40, 28))
    frames = []
    for f in range(12):
        o.reset()
        o.render(f, 1, threads=THREADS)
        frames.append(tuple(o.download(l) for l in range(3)))
    return frames


def _chains(frames, spp):
    chains = np.zeros((8,) + frames[0][0].shape, np.float32)
    s1, s2 = np.zeros_like(frames[0][1]), np.zeros_like(frames[0][2])
    for f in range(spp):
        chains[f % 8] += frames[f][0]
        s1 += frames[f][1]
        s2 += frames[f][2]
    return chains, fr.chain_counts(spp), s1, s2


@pytest.mark.parametrize("spp", (12, 5))
def test_halves_add_up_and_variance_is_one(cornell_frames, spp):
    chains, n_c, s1, s2 = _chains(cornell_frames, spp)
    f32 = fr.features(chains, n_c, s1, s2, np.float32)
    f64 = fr.features(chains, n_c, s1, s2, np.float64)
    assert all(v.dtype == np.float32 for v in f32.values())
    n_a, n_b = int(n_c[0::2].sum()), int(n_c[1::2].sum())
    assert (n_a, n_b) == {12: (6, 6), 5: (3, 2)}[spp] and (f32[fr.FRAMES] == spp).all()
    # the frame-weighted mean of the halves is the image, up to the rounding of the three means (the recombination below is in fp64).  All sums
    # are of non-negative numbers, so every addition and the division err by half an ulp of a value no larger than the result: 3 + 1 half-ulps for
    # each half -- frame-weighted, 4 of the larger one -- and 7 + 1 for the image, 12 half-ulps of the largest of the three: 6 * 2^-23 relative
    # in fp32, 6 * 2^-52 in fp64; 8 * 2^-23 and 8 * 2^-52 are asserted
    for f, eps in ((f64, 8 * 2.0 ** -52), (f32, 8 * 2.0 ** -23)):
        both = (f[fr.HALF_A].astype(np.float64) * n_a + f[fr.HALF_B].astype(np.float64) * n_b) / spp
        scale = np.maximum(np.maximum(f[fr.HALF_A], f[fr.HALF_B]), f[fr.COLOR]).astype(np.float64)
        err = np.abs(both - f[fr.COLOR]) / np.where(scale > 0, scale, 1.0)
        print(f"cornell_box(40, 28) @ {spp}, {f[fr.COLOR].dtype}: halves against the image, max error {err.max():.3g} of the largest (bound {eps:.3g})")
        assert err.max() <= eps
    assert (f32[fr.HALF_A] != f32[fr.HALF_B]).any()  # two different images
    v = f32[fr.VARIANCE]
    assert (v >= 0).all() and v.max() > 0 and np.isfinite(v).all() and (f64[fr.VARIANCE] >= 0).all()
    assert np.abs(v - f64[fr.VARIANCE]).max() <= 1e-5 * f64[fr.VARIANCE].max()
    # the guides are the layer sums over N
    assert np.array_equal(f32[fr.NORMAL], s1 / np.float32(spp)) and np.array_equal(f32[fr.ALBEDO], s2 / np.float32(spp)) and f32[fr.ALBEDO].max() > 0
    # the scene's dark pixels give variances below the smallest normal half: the fp16 tensor holds subnormals
    h = fr.to_f16(v)
    assert ((h > 0) & (h < np.float16(6.1e-5))).any()


def test_one_frame_has_no_second_half_and_no_variance(cornell_frames):
    chains, n_c, s1, s2 = _chains(cornell_frames, 1)
    f = fr.features(chains, n_c, s1, s2, np.float32)
    assert not f[fr.HALF_B].any() and not f[fr.VARIANCE].any()
    assert np.array_equal(f[fr.HALF_A], f[fr.COLOR]) and np.array_equal(f[fr.COLOR], chains[0]) and (f[fr.FRAMES] == 1).all()


def test_variance_spread_of_the_restatement(oracle_mod):
    """The measurement behind the bound of tests/test_gpu_features.py (VARIANCE against rene_estimate_noise's sum_var), on the cases it runs."""
    worst = 0.0
    for name, (scene, args, spp) in fr.SPREAD_CASES.items():
        o = oracle_mod.Oracle(getattr(scenes, scene)(*args))
        chains, n_c, s1, s2 = chains_of(o, spp, threads=THREADS)
        v32 = fr.features(chains, n_c, s1, s2, np.float32)[fr.VARIANCE]
        want = fr.tile_sums(fr.features(chains, n_c, s1, s2, np.float64)[fr.VARIANCE])
        spread = [float((np.abs(fr.tile_sums(v32, d).astype(np.float64) - want) / (np.abs(want) + want.max())).max()) for d in (np.float64, np.float32)]
        print(f"{name}: VARIANCE tile sums, fp32 pixels summed in fp64 / in fp32 against fp64: {spread[0]:.3g} / {spread[1]:.3g}")
        worst = max(worst, *spread)
    assert worst <= fr.VARIANCE_SPREAD, worst


# ---- the build -----------------------------------------------------------------------------------------------------------------------------
def test_unit_is_built_with_the_specified_arithmetic(hip_lib):
    mk = open(os.path.join(ROOT, "rene_amd", "csrc", "Makefile")).read()
    assert "kernels_features.o" in mk.split("OBJS =")[1].splitlines()[0] and "2> kernels_features.res" in mk
    assert "$(HIPCC) $(ROBUSTFLAGS) $(RESFLAGS) -c -o $@ kernels_features.hip" in mk
    assert "$(ROBUSTFLAGS) $(RESFLAGS) $(EXTRA) -c -o var_$(NAME)/kernels_features.o" in mk
    for name in NEW_SYMBOLS:
        assert hasattr(hip_lib, name), name
