"""CPU: the noise estimate's host surface (structs, defaults, the two pure host functions, argument checks) and its specification -- the numpy
restatement of tests/noise_reference.py on a case with a closed form and on the CPU oracle's renders: does the figure defined in
include/rene_hip.h fall as 1 / sqrt(N), and is the variance it is built on calibrated?"""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import noise_reference as nr
from conftest import ROOT
from rene_amd import abi, api, scenes

THREADS = 8
SEEDS = [abi.DEFAULT_SEED + 977 * i for i in range(8)]  # eight master seeds
FLOOR = float(np.float32(nr.DEFAULT_FLOOR))  # the library holds the floor as fp32


def test_structs_match_the_header():
    fields = [("rene_noise_params", "luminance_floor"), ("rene_noise_tile", "n_pixels"), ("rene_noise_estimate", "n_pixels"),
              ("rene_noise_estimate", "sum_weighted_q"), ("rene_noise_estimate", "n_frames"), ("rene_noise_estimate", "luminance_floor"),
              ("rene_noise_estimate", "noise"), ("rene_noise_estimate", "worst_tile")]
    prog = '#include <stdio.h>\n#include "rene_hip.h"\nint main(void){\n'
    for s in ("rene_noise_params", "rene_noise_tile", "rene_noise_estimate"):
        prog += f'printf("%zu\\n", sizeof({s}));\n'
    for s, f in fields:
        prog += f'printf("%zu\\n", offsetof({s}, {f}));\n'
    prog += 'printf("%u\\n", RENE_ABI_VERSION);\nreturn 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = list(map(int, subprocess.check_output([exe]).split()))
    cls = {"rene_noise_params": abi.NoiseParams, "rene_noise_tile": abi.NoiseTile, "rene_noise_estimate": abi.NoiseEstimate}
    assert out[:3] == [C.sizeof(abi.NoiseParams), C.sizeof(abi.NoiseTile), C.sizeof(abi.NoiseEstimate)] == [16, 16, 88]
    for got, (s, f) in zip(out[3:], fields):
        assert got == getattr(cls[s], f).offset, (s, f)
    assert out[-1] == abi.ABI_VERSION == 7  # new symbols and struct_size-carrying structs break no caller
    assert np.dtype(abi.NOISE_TILE_DTYPE).itemsize == C.sizeof(abi.NoiseTile)


def test_defaults_and_null_arguments(hip_lib):
    p = api.noise_params_default()
    assert p.struct_size == C.sizeof(abi.NoiseParams) and p.reserved0 == 0 and p.reserved1 == 0
    assert p.luminance_floor == np.float32(0.01) == np.float32(nr.DEFAULT_FLOOR)
    est = abi.NoiseEstimate()
    assert hip_lib.rene_estimate_noise(None, None, C.byref(est)) == -1 and b"NULL context" in hip_lib.rene_last_error()
    buf = (abi.NoiseTile * 4)()
    assert hip_lib.rene_download_noise_tiles(None, buf, 4) == -1 and hip_lib.rene_last_error()
    assert hip_lib.rene_noise_combine(None, 0, C.byref(est)) == -1 and hip_lib.rene_last_error()
    assert hip_lib.rene_abi_version() == 7


def _part(fig, n_frames=24, n_chains=8, floor=nr.DEFAULT_FLOOR):
    e = abi.NoiseEstimate()
    e.struct_size = C.sizeof(abi.NoiseEstimate)
    for k in ("n_tiles", "n_pixels", "sum_var", "sum_lum", "sum_weighted_q", "noise", "rel_rmse", "worst_tile_noise", "worst_tile"):
        setattr(e, k, fig[k])
    e.n_frames, e.n_chains, e.luminance_floor = n_frames, n_chains, floor
    return e


def test_combine_of_parts_equals_the_whole(hip_lib):
    rng = np.random.default_rng(11)
    ty, tx = 5, 7  # a 200 x 150 image: ragged on both sides
    n = np.full((ty, tx), 1024)
    n[-1, :] = 22 * 32
    n[:, -1] = 8 * 32
    n[-1, -1] = 22 * 8
    b = (rng.uniform(0.0, 2.0, (ty, tx)) * n).astype(np.float32)
    a = (rng.uniform(0.0, 0.05, (ty, tx)) ** 2 * n).astype(np.float32)
    b[1, 2] = a[1, 2] = 0  # a black tile
    whole = nr.figures(a, b, n, FLOOR)
    for count in (2, 3, 8):
        owner = np.arange(ty * tx).reshape(ty, tx) % count
        parts = [_part(nr.figures(a, b, n, FLOOR, owned=owner == r)) for r in range(count)]
        got = api.noise_combine(parts)
        assert got.struct_size == 88 and got.n_frames == 24 and got.n_chains == 8 and got.luminance_floor == np.float32(0.01)
        assert got.n_tiles == whole["n_tiles"] == ty * tx and got.n_pixels == whole["n_pixels"] == int(n.sum())
        assert got.worst_tile == whole["worst_tile"] and got.worst_tile_noise == whole["worst_tile_noise"]
        for k in ("sum_var", "sum_lum", "sum_weighted_q", "noise", "rel_rmse"):
            assert abs(getattr(got, k) - whole[k]) <= 1e-12 * abs(whole[k]), (count, k)
    # the figures are those of the definition, from the additive fields alone (the floor is held as fp32)
    one = api.noise_combine([_part(whole)])
    assert one.noise == pytest.approx(math.sqrt(whole["sum_weighted_q"] / whole["n_pixels"]), rel=1e-14)
    assert one.rel_rmse == pytest.approx(math.sqrt(whole["sum_var"] / whole["n_pixels"]) / (whole["sum_lum"] / whole["n_pixels"] + FLOOR), rel=1e-14)
    # a shard that owns no tile adds nothing and does not become the worst tile
    empty = abi.NoiseEstimate()
    empty.struct_size, empty.n_frames, empty.n_chains, empty.luminance_floor = 88, 24, 8, 0.01
    with_empty = api.noise_combine([empty, _part(whole)])
    assert with_empty.noise == one.noise and with_empty.worst_tile == one.worst_tile and with_empty.n_tiles == one.n_tiles


def test_combine_refuses_mismatched_parts(hip_lib):
    fig = nr.figures(np.full((2, 2), 3.0), np.full((2, 2), 500.0), np.full((2, 2), 1024))

    def code(parts):
        with pytest.raises(api.ReneError) as e:
            api.noise_combine(parts)
        assert str(e.value).split(": ", 1)[1].strip()
        return e.value.code

    assert code([_part(fig), _part(fig, n_frames=32)]) == -1
    assert code([_part(fig), _part(fig, floor=0.02)]) == -1
    bad = _part(fig)
    bad.struct_size = 80
    assert code([_part(fig), bad]) == -1
    assert code([]) == -1
    assert api.noise_combine([_part(fig), _part(fig)]).n_pixels == 2 * 4096


def test_frames_needed(hip_lib):
    def est(n_frames, noise):
        e = abi.NoiseEstimate()
        e.struct_size, e.n_frames, e.noise = 88, n_frames, noise
        return e

    assert api.noise_frames_needed(est(16, 0.5), 0.25) == 64          # twice too noisy: four times the frames
    assert api.noise_frames_needed(est(16, 0.5), 0.125) == 256
    assert api.noise_frames_needed(est(64, 0.375), 0.25) == 144       # 64 * 1.5^2
    assert api.noise_frames_needed(est(10, 0.75), 0.5) == 23          # ceil(22.5)
    assert api.noise_frames_needed(est(100, 0.25), 0.25) == 100       # met exactly
    assert api.noise_frames_needed(est(100, 0.125), 0.5) == 100       # already below the target: at least N
    assert api.noise_frames_needed(est(100, 0.0), 0.5) == 100
    assert api.noise_frames_needed(est(1 << 20, 1.0), 2.0 ** -6) == 0xFFFFFFFF   # 2^32: saturates
    assert api.noise_frames_needed(est(1 << 20, 1.0), 2.0 ** -5) == 1 << 30
    assert api.noise_frames_needed(est(16, 0.5), 1e-30) == 0xFFFFFFFF
    assert api.noise_frames_needed(est(16, 0.5), 0.0) == 0xFFFFFFFF
    assert api.noise_frames_needed(est(16, 0.5), -1.0) == 0xFFFFFFFF
    assert api.noise_frames_needed(est(16, 0.5), float("nan")) == 0xFFFFFFFF
    assert api.noise_frames_needed(est(1 << 40, 0.1), 1.0) == 0xFFFFFFFF         # more frames than a u32 holds
    assert api.next_batch(64, 400, 64, 10000) == 168 and api.next_batch(64, 100, 64, 10000) == 64   # half of what is missing, at least a batch
    assert api.next_batch(64, 401, 64, 10000) == 176 and api.next_batch(64, 0xFFFFFFFF, 64, 100) == 36  # multiples of 8; the cap


def test_restatement_on_a_closed_form():
    """Chains of four frames each whose means are m + d (c - 3.5) in every channel, c = 0 .. 7: lum's weights add up to one, so l = m and
    var = d^2 sum (c - 3.5)^2 / 8 / 7 = 0.75 d^2 in every pixel, q_t = 0.75 d^2 / (m + floor)^2 in every tile, ragged or not."""
    h, w, m, d = 45, 70, 0.8, 0.05
    n_c = np.full(8, 4.0)
    chains = np.stack([np.full((h, w, 3), 4.0 * (m + d * (c - 3.5))) for c in range(8)])
    e = nr.estimate(chains, n_c)
    assert np.abs(e["l"] - m).max() <= 1e-12 and np.abs(e["var"] - 0.75 * d * d).max() <= 1e-12
    assert e["n"].tolist() == [[1024, 1024, 192], [416, 416, 78]] and e["n_pixels"] == h * w and e["n_tiles"] == 6
    want = math.sqrt(0.75) * d / (m + 0.01)
    assert abs(e["noise"] - want) <= 1e-12 and abs(e["rel_rmse"] - want) <= 1e-12 and abs(e["worst_tile_noise"] - want) <= 1e-12
    assert np.abs(e["tile_noise"] - want).max() <= 1e-12
    # unequal chains (12 frames: four chains of two, four of one), the same means: var = sum (n_c / N) (l_c - l)^2 / 7 around the weighted mean
    n_c = np.array([2.0, 2, 2, 2, 1, 1, 1, 1])
    means = m + d * (np.arange(8) - 3.5)
    chains = np.stack([np.full((h, w, 3), n_c[c] * means[c]) for c in range(8)])
    e = nr.estimate(chains, n_c)
    lbar = (n_c * means).sum() / 12
    var = ((n_c / 12) * (means - lbar) ** 2).sum() / 7
    assert np.abs(e["l"] - lbar).max() <= 1e-12 and np.abs(e["var"] - var).max() <= 1e-12
    # five frames: five chains of one, three empty -- k = 5
    n_c = np.array([1.0, 1, 1, 1, 1, 0, 0, 0])
    chains = np.stack([np.full((h, w, 3), n_c[c] * means[c]) for c in range(8)])
    e = nr.estimate(chains, n_c)
    assert np.abs(e["var"] - ((means[:5] - means[:5].mean()) ** 2).sum() / 5 / 4).max() <= 1e-12
    # fp32 follows: the conditioning that lets a device implementation be held to the restatement
    e32 = nr.estimate(chains, n_c, dtype=np.float32)
    assert e32["A"].dtype == np.float32 and abs(e32["noise"] - e["noise"]) <= 1e-5 * e["noise"]


# ---- the specification on oracle renders ---------------------------------------------------------------------------------------------
def _chains_16_and_64(o, seed):
    """The chains of frames 0 .. 15 and of frames 0 .. 63 of one master seed."""
    c16 = np.zeros((8, o.yres, o.xres, 3), np.float32)
    c64 = np.zeros_like(c16)
    for fr in range(64):
        o.reset()
        o.render(fr, 1, seed=seed, threads=THREADS)
        d = o.download(0)
        c64[fr % 8] += d
        if fr < 16:
            c16[fr % 8] += d
    return c16, c64


# the bands are stated, with the oracle's figures they come from, next to nr.LAW_BANDS
LAW = {
    "fog": (lambda: scenes.cornell_fog(64, 64),) + nr.LAW_BANDS["fog"],
    "cornell": (lambda: scenes.cornell_box(100, 70),) + nr.LAW_BANDS["cornell"],
}


@pytest.mark.parametrize("name", list(LAW))
def test_noise_falls_as_one_over_sqrt_n(oracle_mod, name):
    make, band_noise, band_rmse = LAW[name]
    o = oracle_mod.Oracle(make())
    per_pixel = []
    for seed in SEEDS:
        c16, c64 = _chains_16_and_64(o, seed)
        e16, e64 = nr.estimate(c16, np.full(8, 2.0)), nr.estimate(c64, np.full(8, 8.0))
        r_noise, r_rmse = e16["noise"] / e64["noise"], e16["rel_rmse"] / e64["rel_rmse"]
        pp = nr.per_pixel_ratio(e16["l"], e16["var"]) / nr.per_pixel_ratio(e64["l"], e64["var"])
        per_pixel.append(pp)
        print(f"{name} seed {seed:#x}: noise {e16['noise']:.4f} -> {e64['noise']:.4f} ratio {r_noise:.3f}; rel_rmse ratio {r_rmse:.3f}; per-pixel metric ratio {pp:.3f}")
        assert abs(r_noise - 2) <= band_noise, (name, seed, r_noise)
        assert abs(r_rmse - 2) <= band_rmse, (name, seed, r_rmse)
    if name == "fog":  # the finding that rules the per-pixel metric out: on no seed does it come near halving
        assert max(per_pixel) < 2 - band_noise, per_pixel


def test_variance_is_calibrated(oracle_mod):
    """Sum over pixels of the estimated variance of the mean / sum of the empirical variance of the pixel means over the eight seeds, on
    cornell_box(64, 64) at 16 spp.  The oracle gave 0.875 .. 1.209 per seed (deviation 0.209 -> band 0.31; the empirical variance of eight
    samples is itself noisy) and 1.057 for the seeds' mean (0.057 -> 0.085)."""
    o = oracle_mod.Oracle(scenes.cornell_box(64, 64))
    ls, vs = [], []
    for seed in SEEDS:
        chains = np.zeros((8, 64, 64, 3), np.float32)
        for fr in range(16):
            o.reset()
            o.render(fr, 1, seed=seed, threads=THREADS)
            chains[fr % 8] += o.download(0)
        l, v = nr.pixel_stats(chains, np.full(8, 2.0))
        ls.append(l)
        vs.append(v)
    empirical = np.array(ls).var(axis=0, ddof=1).sum()
    ratios = [float(v.sum() / empirical) for v in vs]
    print("calibration per seed:", " ".join(f"{r:.3f}" for r in ratios), f"mean {np.mean(ratios):.3f}")
    assert all(abs(r - 1) <= 0.31 for r in ratios), ratios
    assert abs(np.mean(ratios) - 1) <= 0.085, np.mean(ratios)
