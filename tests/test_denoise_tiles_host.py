"""CPU: the `atrous` denoiser tile by tile (rene_denoise_tiles, include/rene_hip.h) -- its specification, the numpy restatement of
tests/atrous_tiles_reference.py, against the uniform restatement and on a film with an invalid tile; its host surface (ABI mirror, exported
symbol, command line); and the conditioning that sets the bound of the device comparison.

The bound: on oracle chains of the two GPU cases of tests/test_gpu_denoise_tiles.py (cornell_box(161, 130) and cornell_fog(96, 64) under the
five-class schedule) the restatement's fp32 run stays within 4.8e-7 (1 + |value|) of its fp64 run (measured: 4.72e-7 and 1.03e-7).  16 x that is
7.6e-6, smaller than the 2e-5 the uniform filter's device comparison uses: the device is held to that existing 2e-5."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import atrous_reference as ar
import atrous_tiles_reference as at
from conftest import ROOT
from rene_amd import abi, api, scenes

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
THREADS = 8
BOUND = 2e-5  # the device comparison's (tests/test_gpu_denoise_tiles.py)


@pytest.fixture(scope="module")
def cli(hip_lib):
    if not os.path.exists(CLI):
        api.build()
    return CLI


def synthetic(h, w, seed=3):
    rng = np.random.default_rng(seed)
    chains = rng.uniform(0.0, 3.0, (8, h, w, 3)).astype(np.float32)
    chains[:, :, w // 2:] *= 2.5  # an edge
    s1 = rng.normal(0.0, 4.0, (h, w, 3)).astype(np.float32)
    s2 = rng.uniform(0.5, 10.0, (h, w, 3)).astype(np.float32)
    return chains, s1, s2


@pytest.mark.parametrize("frames", [12, 5, 35])  # chains of 2 and 1 frames; three empty chains; 5 and 4 frames
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_equals_the_uniform_one_on_even_counts(frames, dtype):
    h, w = 41, 70
    chains, s1, s2 = synthetic(h, w)
    n_c = at.chain_counts(0, frames)
    want, want_var = ar.denoise(chains, n_c, s1, s2, dtype=dtype)
    got, mean, var, valid = at.denoise_tiles(chains, np.broadcast_to(n_c[:, None, None], (8, h, w)), s1, s2, dtype=dtype)
    assert valid.all() and got.dtype == dtype
    assert np.array_equal(got, want) and np.array_equal(var, want_var)
    assert np.array_equal(mean * dtype(frames), got)  # the radiance is the mean times N, rounded once


def film_with_an_invalid_tile():
    """96 x 64, tiles of 16 / 128 / 19 // 128 / 1 / 128 frames: the middle tile of the bottom row has one frame, in one chain."""
    h, w = 64, 96
    chains, s1, s2 = synthetic(h, w, seed=11)
    frames = np.array([[16, 128, 19], [128, 1, 128]])
    n_c = np.stack([at.per_pixel(np.vectorize(lambda n, g=g: at.chain_counts(0, n)[g])(frames), h, w) for g in range(8)])
    chains = chains * (n_c[..., None] > 0)  # a chain without frames holds zero
    return chains.astype(np.float32), n_c, s1, s2, at.per_pixel(frames, h, w)


def test_an_invalid_tile_is_outside_the_image():
    chains, n_c, s1, s2, frames = film_with_an_invalid_tile()
    out, mean, var, valid = at.denoise_tiles(chains, n_c, s1, s2)
    bad = frames == 1
    assert np.array_equal(valid, ~bad) and bad.sum() == 32 * 32
    s0 = chains.astype(np.float64).sum(0)
    # the invalid pixels come out as the unfiltered input, variance 0
    assert np.array_equal(out[bad], s0[bad]) and np.array_equal(mean[bad], s0[bad] / 1.0) and not var[bad].any()
    assert np.isfinite(out).all() and np.isfinite(mean).all() and (var >= 0).all()
    assert not np.array_equal(out[valid], s0[valid])  # ... and the others are filtered
    # no valid pixel's result changes when the invalid tile's contents are replaced by NaN: its pixels are skipped, not weighted with zero
    c2, t1, t2 = chains.copy(), s1.copy(), s2.copy()
    c2[:, bad], t1[bad], t2[bad] = np.nan, np.nan, np.nan
    out2, mean2, var2, _ = at.denoise_tiles(c2, n_c, t1, t2)
    assert np.array_equal(out2[valid], out[valid]) and np.array_equal(mean2[valid], mean[valid]) and np.array_equal(var2, var)
    # the variance plane of the valid tiles is the uniform restatement's at the tile's count, tile by tile
    for n in (16, 19, 128):
        _, uvar = ar.denoise(chains, at.chain_counts(0, n), s1, s2)
        m = frames == n
        assert np.array_equal(var[m], uvar[m]), n
    # the radiance is the mean times the pixel's own count
    assert np.array_equal(out[valid], (mean * frames[..., None])[valid])


def test_a_film_without_frames_and_one_with_a_lone_valid_tile():
    chains, n_c, s1, s2, frames = film_with_an_invalid_tile()
    lone = frames == 19
    n2 = n_c * lone  # every other tile: no frames at all
    c2 = chains * lone[None, ..., None]
    out, mean, var, valid = at.denoise_tiles(c2, n2, s1, s2)
    assert np.array_equal(valid, lone) and np.isfinite(out).all() and not out[~lone].any() and not mean[~lone].any()
    # the lone tile is filtered as an image of its own: nothing outside it is a tap
    rows, cols = np.where(lone.any(1))[0], np.where(lone.any(0))[0]
    sl = (slice(rows[0], rows[-1] + 1), slice(cols[0], cols[-1] + 1))
    want, want_var = ar.denoise(chains[(slice(None),) + sl], at.chain_counts(0, 19), s1[sl], s2[sl])
    assert np.array_equal(out[sl], want) and np.array_equal(var[sl], want_var)


def test_the_schedule_of_the_gpu_tests():
    for xres, yres in ((161, 130), (96, 64)):
        classes = at.tile_classes(xres, yres)
        assert set(classes.ravel()) == set("ABCDE")
    assert classes.shape == (2, 3) and at.tile_classes(161, 130).shape == (5, 6)
    assert sorted(at.CLASS_FRAMES.values()) == list(np.cumsum((0,) + at.LAUNCHES))
    calls = []
    fake = type("R", (), {"set_active_tiles": lambda self, m: calls.append(("mask", int(m.sum()))), "render": lambda self, f, n: calls.append((f, n))})()
    at.run_schedule(fake, classes, cuts=3)
    renders = [c for c in calls if c[0] != "mask"]
    assert sum(n for _, n in renders) == 35 and [f for f, _ in renders] == list(np.cumsum([0] + [n for _, n in renders])[:-1])
    assert [c[1] for c in calls if c[0] == "mask"] == [4, 3, 2, 1]  # 3 x 2 tiles, classes A B C / D E A: one class fewer each time


def test_abi_mirror_and_exported_symbol(hip_lib):
    assert abi.DENOISED_MEAN == 2 and (abi.DENOISED_RADIANCE, abi.DENOISED_VARIANCE) == (0, 1)
    assert "rene_denoise_tiles" in abi.EXPORTED_SYMBOLS and hasattr(hip_lib, "rene_denoise_tiles")
    assert hip_lib.rene_denoise_tiles.argtypes and hip_lib.rene_denoise_tiles.argtypes == hip_lib.rene_denoise.argtypes
    assert hip_lib.rene_denoise_tiles(None, None) == -1 and b"rene_denoise_tiles: NULL context" in hip_lib.rene_last_error()
    header = open(os.path.join(ROOT, "include", "rene_hip.h")).read()
    assert re.search(r"int rene_denoise_tiles\(rene_ctx\* ctx, const rene_denoise_params\* params\);", header)
    assert re.search(r"RENE_DENOISED_MEAN = 2\b", header)
    assert abi.ABI_VERSION == 7 and C.sizeof(abi.DenoiseParams) == 32  # additive: the version and the params struct are what they were
    assert callable(api.Renderer.denoise_tiles)


def test_cli_accepts_atrous_tiles(cli, tmp_path):
    missing = str(tmp_path / "missing.pbrt")
    for extra in ([], ["--adaptive", "--target-noise", "0.1"]):  # with or without --adaptive: past option parsing, the loader's error
        r = subprocess.run([cli, "--denoiser", "atrous-tiles", *extra, missing], capture_output=True, text=True)
        assert r.returncode == 1 and "invalid --denoiser" not in r.stderr and "cannot be combined" not in r.stderr, (r.returncode, r.stderr)
        assert r.stdout.strip() and "denoiser was enabled" not in r.stderr
    for args in (["--denoiser", "atrous-tiles", "--gpus", "2"], ["--gpus", "2", "--denoiser", "atrous-tiles"]):
        r = subprocess.run([cli, *args, "x.pbrt"], capture_output=True, text=True)
        assert r.returncode == 2 and "--denoiser atrous-tiles" in r.stderr and "--gpus" in r.stderr, r.stderr
    r = subprocess.run([cli, "--denoiser", "atrous-tiles", "--robust", "x.pbrt"], capture_output=True, text=True)
    assert r.returncode == 2 and "--robust" in r.stderr and "atrous-tiles" in r.stderr, r.stderr
    r = subprocess.run([cli, "--denoiser", "bogus", "x.pbrt"], capture_output=True, text=True)
    assert r.returncode == 2 and "invalid --denoiser bogus" in r.stderr
    r = subprocess.run([cli, "--adaptive", "--target-noise", "0.1", "--denoiser", "atrous", "x.pbrt"], capture_output=True, text=True)
    assert r.returncode == 2 and "atrous-tiles" in r.stderr  # still refused, and the message names the spelling that works
    r = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert "none|optix|oidn|atrous|atrous-tiles" in r.stderr


def test_the_two_units_share_their_kernels_text():
    """Every instantiation of the denoiser's prepare, pass and finalize kernels comes from one definition in one unit, and the tap from one header,
    so a valid pixel's arithmetic cannot drift apart between rene_denoise, rene_denoise_tiles, the tile shards and the trimmed prepare."""
    src = os.path.join(ROOT, "rene_amd", "csrc")
    sources = {f: open(os.path.join(src, f)).read() for f in os.listdir(src) if re.search(r"denoise|atrous", f) and f.endswith((".hip", ".h", ".inc"))}
    assert sorted(sources) == ["atrous_filter.h", "kernels_denoise.hip", "kernels_denoise_trim.hip"]
    assert [f for f, text in sources.items() if "__expf" in text] == ["atrous_filter.h"]  # the tap lives in the shared header
    everything = "\n".join(sources.values())
    for kernel in ("denoise_prepare_kernel", "atrous_pass_kernel", "denoise_finalize_kernel"):
        assert len(re.findall(r"__global__[^;{]*?\b" + kernel + r"\(", everything)) == 1, kernel
    assert "robust_prepare_pixel" not in everything and "ATROUS_" not in everything
    mk = open(os.path.join(src, "Makefile")).read()
    assert "kernels_denoise.o" in mk.split("OBJS =")[1].splitlines()[0] and "2> kernels_denoise.res" in mk
    assert "atrous_filter.h" in mk.split("HDRS =")[1].splitlines()[0] and "atrous_kernels.inc" not in mk
    variant = mk.split("variant:")[1]
    assert re.search(r"for u in [^;]*\bkernels_denoise\b", variant) and "kernels_denoise_trim.hip" in variant  # `make variant` builds them too
    assert not re.search(r"kernels_denoise_(tiles|shard|robust)", mk)


@pytest.fixture(scope="module")
def oracle_films(oracle_mod):
    films = {}

    def get(name):
        if name not in films:
            make = {"cornell": lambda: scenes.cornell_box(161, 130), "fog": lambda: scenes.cornell_fog(96, 64)}[name]
            o = oracle_mod.Oracle(make())
            by = at.chains_by_count(o, set(at.CLASS_FRAMES.values()), threads=THREADS)
            films[name] = at.compose({c: by[n] for c, n in at.CLASS_FRAMES.items()}, at.tile_classes(o.xres, o.yres), o.yres, o.xres)
        return films[name]
    return get


@pytest.mark.parametrize("name", ["cornell", "fog"])
def test_restatement_is_conditioned_for_the_device_bound(oracle_films, name):
    """The fp32 run of the restatement stays within BOUND / 16 of the fp64 run on oracle chains of the GPU cases (measured 4.72e-7 and 1.03e-7 of
    1 + |value|, on the mean image): what justifies holding the device to BOUND."""
    film = oracle_films(name)
    out64, mean64, var64, valid = at.denoise_tiles(*film)
    out32, mean32, _, _ = at.denoise_tiles(*film, dtype=np.float32)
    spread = float((np.abs(mean32 - mean64) / (1 + np.abs(mean64))).max())
    print(f"{name}: fp32 vs fp64 {spread:.3g} of 1 + |value|; {valid.mean():.2f} of the pixels valid")
    assert mean32.dtype == np.float32 and np.isfinite(out64).all() and (var64 >= 0).all()
    assert 0.3 < valid.mean() < 0.8
    assert 16 * spread <= BOUND, (name, spread)
