"""GPU: the `atrous` denoiser tile by tile (rene_denoise_tiles) -- bit for bit rene_denoise where the tiles are even; against its specification,
the numpy restatement of tests/atrous_tiles_reference.py fed with the device's own frame chains, where they are not (two classes of invalid
tiles included); its contract (read-only, deterministic, independent of the cut, the same from loaded chains, refusing what it cannot do); its
quality on an adaptive job; and through the command line.

BOUND: the restatement's fp32 run stays within 4.72e-7 (1 + |value|) of its fp64 run on oracle chains of the two specification cases
(tests/test_denoise_tiles_host.py); 16 x that is 7.6e-6, below the 2e-5 of tests/test_gpu_denoise.py, which therefore stays."""
import os
import subprocess

import numpy as np
import pytest

import atrous_reference as ar
import atrous_tiles_reference as at
from conftest import ROOT
from rene_amd import abi, api, loader, scenes

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
BOUND = 2e-5


def results(r):
    return (r.download_denoised(channels=4), r.download_denoised(abi.DENOISED_VARIANCE), r.download_denoised(abi.DENOISED_MEAN, channels=4))


def assert_even_context_equals_denoise(r, n, label):
    r.denoise()
    want, want_var, want_mean = results(r)
    r.denoise_tiles()
    got, got_var, got_mean = results(r)
    assert np.array_equal(got, want) and np.array_equal(got_var, want_var), label
    assert np.array_equal(got_mean, want_mean), label  # RENE_DENOISED_MEAN serves either call
    assert np.array_equal(got_mean * np.float32(n), got), label  # ... and the radiance is the mean times N, rounded once
    assert want.any() and want_var.any() and not got[..., 3].any()


EVEN_CASES = {
    "cornell": (lambda: scenes.cornell_box(100, 70), 12),        # ragged tiles, chains of 2 and 1 frames
    "dragon": (lambda: scenes.dragon_class(240, 136), 16),       # BVH traversal-restart kernel
    "cornell-at-size": (lambda: scenes.cornell_box(1283, 821), 8),  # many workgroups per XCD, ragged edges
}


@pytest.mark.parametrize("name", list(EVEN_CASES))
def test_even_context_equals_denoise_bit_for_bit(name, monkeypatch):
    make, n = EVEN_CASES[name]
    with api.Renderer(make()) as r:
        r.render(0, n)
        assert_even_context_equals_denoise(r, n, name)
        if name != "cornell":
            return
        for stage_max in ("0", "4"):  # every pass direct; steps 1, 2, 4 staged in LDS
            monkeypatch.setenv("RENE_DENOISE_STAGE_MAX", stage_max)
            for columns in (None, "0", "3"):  # the default order of the workgroups' tiles; launch order; ragged super-columns
                if columns is None:
                    monkeypatch.delenv("RENE_DENOISE_TILE_COLUMNS", raising=False)
                else:
                    monkeypatch.setenv("RENE_DENOISE_TILE_COLUMNS", columns)
                assert_even_context_equals_denoise(r, n, (name, stage_max, columns))


def test_even_context_with_tiles_switched_off():
    with api.Renderer(scenes.cornell_box(100, 70)) as r:
        r.render(0, 12)
        r.set_active_tiles(at.tile_classes(100, 70) != "A")  # off, but every N_t is still 12
        assert_even_context_equals_denoise(r, 12, "switched off")
        r.render(12, 4)  # now uneven: 12 and 16
        with pytest.raises(api.ReneError) as e:
            r.denoise()
        assert e.value.code == -4
        r.denoise_tiles()
        assert np.isfinite(r.download_denoised()).all()


# ---- the specification on uneven tiles ---------------------------------------------------------------------------------------------------------
SPEC_CASES = {
    "cornell": lambda: scenes.cornell_box(161, 130),  # 30 tiles, the last column one pixel wide
    "fog": lambda: scenes.cornell_fog(96, 64),        # volpath; 6 tiles
}
_spec = {}


def device_chain_layers(r, spp):
    """All three layers of the chains a job of frames 0 .. spp - 1 leaves on the device, (8, 3, H, W, 3): for chain c, reset, render every frame
    f = c (mod 8) on its own, download -- the other chains hold 0 and adding 0 is exact (the device_chains of test_gpu_denoise.py, every layer)."""
    chains = np.zeros((8, 3, r.yres, r.xres, 3), np.float32)
    for c in range(8):
        r.reset()
        for f in range(c, spp, 8):
            r.render(f, 1)
        for l in range(3):
            chains[c, l] = r.download(l)
    return chains


def spec(name):
    """Computed once per case and left unchanged: the uniform jobs of every class's N_t (chains with all layers, rene_denoise's variance plane), the
    film composed of them tile by tile, the restatement's result on it, and the device's on the masked schedule."""
    if name in _spec:
        return _spec[name]
    s = {}
    with api.Renderer(SPEC_CASES[name]()) as r:
        h, w = r.yres, r.xres
        classes = at.tile_classes(w, h)
        parts, s["uniform_var"] = {}, {}
        for cl, n in at.CLASS_FRAMES.items():
            full = device_chain_layers(r, n)
            s1, s2 = full[0, 1].copy(), full[0, 2].copy()
            for c in range(1, 8):  # ((c0 + c1) + ...) + c7: the resolved layers
                s1 += full[c, 1]
                s2 += full[c, 2]
            parts[cl] = (full[:, 0], at.chain_counts(0, n), s1, s2, full)
            if n >= 2:
                r.reset()
                r.render(0, n)
                r.denoise()
                s["uniform_var"][n] = r.download_denoised(abi.DENOISED_VARIANCE)
        chains, n_c, s1, s2 = at.compose({cl: p[:4] for cl, p in parts.items()}, classes, h, w)
        index = at.per_pixel(np.vectorize("ABCDE".index)(classes), h, w)
        loaded = np.zeros((8, 3, h, w, 3), np.float32)
        for i, cl in enumerate("ABCDE"):
            loaded[:, :, index == i] = parts[cl][4][:, :, index == i]
        s.update(classes=classes, frames=at.per_pixel(at.class_frames(classes), h, w), film=(chains, n_c, s1, s2), loaded=loaded)
        s["want"] = at.denoise_tiles(chains, n_c, s1, s2)
        r.reset()
        at.run_schedule(r, classes)
        s["layers"] = [r.download(l) for l in range(3)]
        s["plain_mean"] = r.download_mean(0)
        s["tile_frames"] = r.tile_frames()
        r.denoise_tiles()
        s["got"] = results(r)
        s["after"] = ([r.download(l) for l in range(3)], r.tile_frames())
        r.denoise_tiles()
        s["again"] = results(r)
        with pytest.raises(api.ReneError) as e:
            r.denoise()
        s["denoise_code"] = e.value.code
    _spec[name] = s
    return s


@pytest.mark.parametrize("name", list(SPEC_CASES))
def test_device_equals_specification_on_uneven_tiles(name):
    s = spec(name)
    chains, n_c, s1, s2 = s["film"]
    acc = chains[0].copy()
    for c in range(1, 8):
        acc += chains[c]
    assert np.array_equal(acc, s["layers"][0]) and np.array_equal(s1, s["layers"][1]) and np.array_equal(s2, s["layers"][2])  # the composed film is the job's
    assert np.array_equal(s["tile_frames"], at.class_frames(s["classes"]))
    want, want_mean, want_var, valid = s["want"]
    got, got_var, got_mean = (s["got"][0][..., :3], s["got"][1], s["got"][2][..., :3])
    frames = s["frames"]
    assert np.array_equal(valid, frames >= 2) and 0.3 < valid.mean() < 0.8
    assert np.isfinite(got).all() and np.isfinite(got_mean).all() and np.isfinite(got_var).all()
    # within the bound of the restatement, on the mean image (every tile in the same unit)
    err = np.abs(got_mean.astype(np.float64) - want_mean) / (1 + np.abs(want_mean))
    y, x, ch = np.unravel_index(int(err.argmax()), err.shape)
    verr = np.abs(got_var.astype(np.float64) - want_var) - BOUND * np.abs(want_var)
    print(f"{name}: mean max err {err.max():.3g} of 1 + |value| at pixel ({x}, {y}) channel {ch} (device {got_mean[y, x, ch]:.6g}, restatement "
          f"{want_mean[y, x, ch]:.6g}, N_t {frames[y, x]}); variance max |diff| - rtol |v| = {verr.max():.3g} against atol {BOUND * want_var.max():.3g}")
    assert err.max() <= BOUND, (name, float(err.max()), (int(x), int(y), int(ch)))
    assert (verr <= BOUND * want_var.max()).all(), (name, float(verr.max()))
    rerr = np.abs(got.astype(np.float64) - want) / np.maximum(frames, 1)[..., None] / (1 + np.abs(want_mean))
    assert rerr.max() <= BOUND, (name, float(rerr.max()))
    # the variance plane, tile by tile, is the uniform context's rene_denoise variance at N_t; 0 on invalid pixels
    for n, uvar in s["uniform_var"].items():
        m = frames == n
        assert m.any() and np.array_equal(got_var[m], uvar[m]), (name, n)
    assert not got_var[~valid].any()
    # invalid pixels hand out the unfiltered image, valid ones do not
    assert np.array_equal(got[~valid], s["layers"][0][~valid]) and np.array_equal(got_mean[~valid], s["plain_mean"][~valid])
    assert got[frames == 1].any() and not got[frames == 0].any()
    assert not np.array_equal(got[valid], s["layers"][0][valid])
    # the radiance is the mean times the tile's N_t, rounded once
    assert np.array_equal(got[valid], (got_mean * frames[..., None].astype(np.float32))[valid])
    assert not s["got"][0][..., 3].any() and not s["got"][2][..., 3].any()


@pytest.mark.parametrize("name", list(SPEC_CASES))
def test_read_only_deterministic_and_refused_by_denoise(name):
    s = spec(name)
    layers, frames = s["after"]
    for l in range(3):
        assert np.array_equal(layers[l], s["layers"][l]), l
    assert np.array_equal(frames, s["tile_frames"])
    for a, b in zip(s["got"], s["again"]):
        assert np.array_equal(a, b)
    assert s["denoise_code"] == -4  # rene_denoise still refuses the context


def test_independent_of_the_cut_and_the_same_from_loaded_chains():
    name = "cornell"
    s = spec(name)
    with api.Renderer(SPEC_CASES[name]()) as r:
        at.run_schedule(r, s["classes"], cuts=3)  # every launch in up to three render calls
        assert np.array_equal(r.tile_frames(), s["tile_frames"])
        r.denoise_tiles()
        for a, b in zip(results(r), s["got"]):
            assert np.array_equal(a, b)
        r.reset()
        r.load_chains(s["loaded"], 0, 35, tile_frames=s["tile_frames"])
        for l in range(3):
            assert np.array_equal(r.download(l), s["layers"][l]), l
        r.denoise_tiles()
        for a, b in zip(results(r), s["got"]):
            assert np.array_equal(a, b)


def test_errors_leave_the_context_usable():
    sc = scenes.cornell_box(96, 64)
    classes = at.tile_classes(96, 64)

    def code(fn):
        with pytest.raises(api.ReneError) as e:
            fn()
        assert str(e.value).split(": ", 1)[1].strip()  # a message
        return e.value.code

    with api.Renderer(sc, shard_mode=abi.SHARD_TILES, shard_rank=0, shard_count=2) as r:
        r.render(0, 8)
        assert code(r.denoise_tiles) == -4  # RENE_ERR_UNSUPPORTED
        assert r.download(0).max() > 0
    with api.Renderer(sc) as r:
        assert code(r.denoise_tiles) == -1  # no frames: no valid tile
        r.render(0, 1)
        assert code(r.denoise_tiles) == -1  # one frame: one chain, in every tile
        assert code(lambda: r.download_denoised(abi.DENOISED_MEAN)) == -1  # nothing to download yet
        r.reset()
        at.run_schedule(r, classes)
        r.denoise_tiles()
        before = results(r)
        assert code(lambda: r.denoise_tiles(iterations=0)) == -1
        assert code(lambda: r.denoise_tiles(iterations=9)) == -1
        assert code(lambda: r.denoise_tiles(sigma_luminance=float("nan"))) == -1
        assert code(lambda: r.denoise_tiles(albedo_floor=0.0)) == -1
        assert code(lambda: r.download_denoised(what=7)) == -1
        assert code(lambda: r.download_denoised(abi.DENOISED_MEAN, channels=1)) == -1
        assert code(r.denoise) == -4
        for a, b in zip(results(r), before):  # a refusal leaves the previous result downloadable
            assert np.array_equal(a, b)
        r.denoise_tiles(iterations=1, sigma_luminance=2.0)  # ... and the context usable
        assert not np.array_equal(r.download_denoised(channels=4), before[0])
        ptr, n = r.denoised_buffer()
        assert ptr and n == 96 * 64 * 4
        r.reset()
        assert code(lambda: r.download_denoised(abi.DENOISED_MEAN)) == -1  # reset: no result
        r.set_active_tiles(np.zeros(classes.shape))
        r.render(0, 8)  # no tile active: nothing rendered
        assert code(r.denoise_tiles) == -1  # no valid owned tile at all
    with api.Renderer(sc) as r:  # an exchange consumes the chains
        r.comm_init(1, 0, api.comm_unique_id())
        r.render(0, 16)
        r.denoise_tiles()
        r.gather_tiles(0)
        assert code(r.denoise_tiles) == -4  # RENE_ERR_UNSUPPORTED, until the reset
        r.reset()
        r.render(0, 16)
        r.denoise_tiles()
        assert np.isfinite(r.download_denoised(abi.DENOISED_MEAN)).all()


QUALITY_FRAMES = np.array([[16, 128, 19], [128, 11, 128]])
QUALITY_LAUNCHES = ((11, (1, 1)), (5, (0, 0)), (3, (0, 2)), (109, None))


@pytest.mark.parametrize("name", ["cornell", "fog"])
def test_quality_on_an_adaptive_job(name):
    """relMSE(denoised mean) <= 0.5 relMSE(download_mean) against an independent 2048-frame device render from frame 100000 (the restatement on
    oracle renders of exactly this layout measured ratios of 0.277 and 0.049)."""
    make = {"cornell": lambda: scenes.cornell_box(96, 64), "fog": lambda: scenes.cornell_fog(96, 64)}[name]
    with api.Renderer(make()) as r:
        r.render(100000, 2048)
        ref = r.download(0).astype(np.float64) / 2048
        r.reset()
        mask, done = np.ones((2, 3), bool), 0
        for n, drop in QUALITY_LAUNCHES:
            r.render(done, n)
            done += n
            if drop:
                mask[drop] = False
                r.set_active_tiles(mask)
        assert np.array_equal(r.tile_frames(), QUALITY_FRAMES)
        noisy = r.download_mean(0).astype(np.float64)
        r.denoise_tiles()
        out = r.download_denoised(abi.DENOISED_MEAN).astype(np.float64)
    e0, e1 = ar.relmse(noisy, ref), ar.relmse(out, ref)
    print(f"{name}: relMSE noisy {e0:.4g} denoised {e1:.4g} ratio {e1 / e0:.3f}; energy ratio {out.mean() / noisy.mean():.3f}")
    assert e1 <= 0.5 * e0, (name, e0, e1)


def test_cli_writes_the_denoised_image(hip_lib, tmp_path):
    from PIL import Image
    p = tmp_path / "scene.pbrt"
    p.write_text(loader.scene_to_pbrt(scenes.cornell_box(96, 64)))

    def run(out, *extra):
        r = subprocess.run([CLI, str(p), "--out", str(tmp_path / out), *extra], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 0, r.stderr
        return r.stderr

    png = lambda name: np.asarray(Image.open(tmp_path / name).convert("RGB"))
    # without --adaptive: the image of --denoiser atrous, byte for byte
    err = run("t.png", "--spp", "16", "--denoiser", "atrous-tiles")
    assert "INFO atrous denoiser:" in err and "0 of 6 tiles invalid" in err and "denoiser was enabled" not in err
    run("a.png", "--spp", "16", "--denoiser", "atrous")
    assert (tmp_path / "t.png").read_bytes() == (tmp_path / "a.png").read_bytes()
    # with --adaptive: to_rgb8 of the denoised mean of the same job
    # (the tile noise of this scene is 0.40 - 0.56 after 16 frames and 0.27 - 0.40 after 32: two tiles stop at 16, the others at 32)
    target = 0.45
    job = ("--spp", "64", "--batch", "16", "--adaptive", "--dilate", "0", "--target-noise", str(target))
    err = run("ad.png", *job, "--denoiser", "atrous-tiles")
    assert "INFO atrous denoiser:" in err and "tiles invalid" in err
    run("plain.png", *job)
    with api.Renderer(loader.load_pbrt(str(p))) as rr:
        frames, _ = rr.render_adaptive(target=target, max_frames=64, batch=16, dilate=0)
        assert len(np.unique(frames)) > 1, frames  # the job is uneven: what the option is for
        plain = api.to_rgb8(rr.download_mean(0), 1)
        rr.denoise_tiles()
        want = api.to_rgb8(rr.download_denoised(abi.DENOISED_MEAN), 1)
    assert np.array_equal(png("plain.png"), plain)  # the same job
    assert np.array_equal(png("ad.png"), want) and not np.array_equal(want, plain)
