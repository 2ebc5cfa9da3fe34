"""GPU: the `atrous` denoiser (rene_denoise) against its specification -- the numpy restatement of tests/atrous_reference.py fed with the
device's own frame chains, rebuilt through the public ABI -- and its contract: read-only, deterministic, independent of how a job is cut
into calls, refusing what it cannot do, and through the command line."""
import os
import subprocess

import numpy as np
import pytest

import atrous_reference as ar
from conftest import ROOT
from rene_amd import abi, api, loader, scenes

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
BOUND = 2e-5  # 16 x the largest fp32-vs-fp64 spread of the restatement (1.3e-6): v_rcp_f32 / v_sqrt_f32 / v_exp_f32 and the order of the 25-tap sums


def device_chains(r, spp):
    """The chains a job of frames 0 .. spp - 1 leaves on the device: for chain c, reset, render every frame f = c (mod 8) on its own, download
    -- the other chains hold 0 and adding 0 is exact, so the download IS C_c bit for bit."""
    chains = np.zeros((8, r.yres, r.xres, 3), np.float32)
    n_c = np.zeros(8)
    for c in range(8):
        r.reset()
        for f in range(c, spp, 8):
            r.render(f, 1)
            n_c[c] += 1
        chains[c] = r.download(0)
    return chains, n_c


def check_against_restatement(r, spp, label):
    chains, n_c = device_chains(r, spp)
    r.reset()
    r.render(0, spp)
    s0, s1, s2 = r.download(0), r.download(1), r.download(2)
    acc = chains[0].copy()
    for c in range(1, 8):
        acc += chains[c]
    assert np.array_equal(acc, s0), label  # the rebuilt chains are the job's chains
    r.denoise()
    got, got_var = r.download_denoised().astype(np.float64), r.download_denoised(abi.DENOISED_VARIANCE).astype(np.float64)
    want, want_var = ar.denoise(chains, n_c, s1, s2)
    err = np.abs(got / spp - want / spp) / (1 + np.abs(want / spp))
    y, x, ch = np.unravel_index(int(err.argmax()), err.shape)
    verr = np.abs(got_var - want_var) - BOUND * np.abs(want_var)
    print(f"{label}: radiance max err {err.max():.3g} of 1 + |value| at pixel ({x}, {y}) channel {ch} (device {got[y, x, ch] / spp:.6g}, restatement "
          f"{want[y, x, ch] / spp:.6g}); variance max |diff| - rtol |v| = {verr.max():.3g} against atol {BOUND * want_var.max():.3g}; "
          f"energy ratio {got.mean() / s0.astype(np.float64).mean():.3f}")
    assert np.isfinite(got).all()
    assert err.max() <= BOUND, (label, float(err.max()), (int(x), int(y), int(ch)))
    assert (verr <= BOUND * want_var.max()).all(), (label, float(verr.max()), float(want_var.max()))
    return got


SPEC_CASES = {
    "cornell": (lambda: scenes.cornell_box(100, 70), 12, 0),       # ragged tiles, chains of 2 and 1 frames
    "zoo": (lambda: scenes.material_zoo(192, 128), 32, 0),         # textures, environment map, every material
    "fog": (lambda: scenes.cornell_fog(96, 64), 32, 0),            # volpath
    "dragon": (lambda: scenes.dragon_class(240, 136), 16, 0),      # BVH traversal-restart kernel
    "dragon-wavefront": (lambda: scenes.dragon_class(240, 136), 16, abi.FLAG_WAVEFRONT),
}


@pytest.mark.parametrize("name", list(SPEC_CASES))
def test_device_equals_specification(name):
    make, spp, flags = SPEC_CASES[name]
    with api.Renderer(make(), flags=flags) as r:
        check_against_restatement(r, spp, name)


def test_device_equals_specification_at_size():
    """More than 2^20 pixels, neither side a multiple of 32: most taps of steps 8 and 16 land inside the image, many workgroups meet tile
    borders, and the index arithmetic sees real sizes."""
    with api.Renderer(scenes.cornell_box(1283, 821)) as r:
        check_against_restatement(r, 8, "cornell 1283x821")


def test_staged_and_direct_passes_agree():
    """The LDS-staged kernels (steps 1, 2, 4) and the direct kernel do the same arithmetic in the same order: whichever the library picks, the
    image is the same bit for bit (RENE_DENOISE_STAGE_MAX and RENE_DENOISE_TILE_COLUMNS are the A/B knobs of DESIGN.md section 4c)."""
    with api.Renderer(scenes.material_zoo(203, 77)) as r:
        r.render(0, 16)
        r.denoise()
        want = r.download_denoised(channels=4)
        try:
            for stage_max in ("0", "1", "2"):
                os.environ["RENE_DENOISE_STAGE_MAX"] = stage_max
                r.denoise()
                assert np.array_equal(r.download_denoised(channels=4), want), stage_max
                # ... and in whichever order the workgroups take the tiles (launch order; super-columns of 3 tiles, ragged; of more tiles than a row has)
                for columns in ("0", "3", "64"):
                    os.environ["RENE_DENOISE_TILE_COLUMNS"] = columns
                    r.denoise()
                    assert np.array_equal(r.download_denoised(channels=4), want), (stage_max, columns)
                del os.environ["RENE_DENOISE_TILE_COLUMNS"]
        finally:
            os.environ.pop("RENE_DENOISE_STAGE_MAX", None)
            os.environ.pop("RENE_DENOISE_TILE_COLUMNS", None)
        assert (want[..., 3] == 0).all()


def test_read_only_and_deterministic():
    s = scenes.cornell_box(100, 70)
    with api.Renderer(s) as r, api.Renderer(s) as plain:
        r.render(0, 12)
        plain.render(0, 12)
        before = [r.download(l) for l in range(3)]
        r.denoise()
        first = r.download_denoised()
        for l in range(3):
            assert np.array_equal(r.download(l), before[l]) and np.array_equal(plain.download(l), before[l])
        r.denoise()
        assert np.array_equal(r.download_denoised(), first)
        var = r.download_denoised(abi.DENOISED_VARIANCE)
        assert var.shape == (70, 100) and (var >= 0).all() and var.max() > 0
        ptr, n = r.denoised_buffer()
        assert ptr and n == 100 * 70 * 4
        r.render(12, 8)  # later frames are what they are without the call
        plain.render(12, 8)
        for l in range(3):
            assert np.array_equal(r.download(l), plain.download(l))
        r.denoise()
        plain.denoise()
        assert np.array_equal(r.download_denoised(), plain.download_denoised())
    with api.Renderer(s) as a, api.Renderer(s) as b:  # the chains' cut independence carried through
        a.render(0, 32)
        for first_frame, n in ((0, 5), (5, 20), (25, 7)):
            b.render(first_frame, n)
        a.denoise()
        b.denoise()
        assert np.array_equal(a.download_denoised(), b.download_denoised())
        assert np.array_equal(a.download_denoised(abi.DENOISED_VARIANCE), b.download_denoised(abi.DENOISED_VARIANCE))


QUALITY_CASES = {
    "cornell": (lambda: scenes.cornell_box(100, 70), 12),
    "zoo": (lambda: scenes.material_zoo(192, 128), 32),
    "veach": (lambda: scenes.veach_mis(160, 90), 32),
    "fog": (lambda: scenes.cornell_fog(96, 64), 32),
}


@pytest.mark.parametrize("name", list(QUALITY_CASES))
def test_quality_on_the_device(name):
    """relMSE(denoised) <= 0.5 relMSE(noisy) against an independent 2048-spp GPU render from frame 100000 (the restatement on oracle renders
    measured ratios of 0.06 - 0.25)."""
    make, spp = QUALITY_CASES[name]
    with api.Renderer(make()) as r:
        r.render(100000, 2048)
        ref = r.download(0).astype(np.float64) / 2048
        r.reset()
        r.render(0, spp)
        noisy = r.download(0).astype(np.float64) / spp
        r.denoise()
        out = r.download_denoised().astype(np.float64) / spp
    e0, e1 = ar.relmse(noisy, ref), ar.relmse(out, ref)
    print(f"{name}: relMSE noisy {e0:.4g} denoised {e1:.4g} ratio {e1 / e0:.3f}; energy ratio {out.mean() / noisy.mean():.3f}")
    assert e1 <= 0.5 * e0, (name, e0, e1)


def test_errors_leave_the_context_usable():
    s = scenes.cornell_box(64, 48)

    def code(fn):
        with pytest.raises(api.ReneError) as e:
            fn()
        assert str(e.value).split(": ", 1)[1].strip()  # a message
        return e.value.code

    with api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=0, shard_count=2) as r:
        r.render(0, 8)
        assert code(r.denoise) == -4  # RENE_ERR_UNSUPPORTED
        assert r.download(0).max() > 0
    with api.Renderer(s) as r:
        assert code(r.denoise) == -1  # no frames
        r.render(0, 1)
        assert code(r.denoise) == -1  # one frame: one chain
        assert code(r.download_denoised) == -1  # nothing to download yet
        assert code(r.denoised_buffer) == -1
        r.render(8, 1)
        assert code(r.denoise) == -1  # two frames, both in chain 0
        r.render(1, 7)
        assert code(lambda: r.denoise(iterations=0)) == -1
        assert code(lambda: r.denoise(iterations=9)) == -1
        assert code(lambda: r.denoise(sigma_luminance=float("nan"))) == -1
        assert code(lambda: r.denoise(albedo_floor=0.0)) == -1
        assert code(lambda: r.denoise(sigma_normal2=float("inf"))) == -1
        assert code(lambda: r.download_denoised(what=7)) == -1
        assert code(lambda: r.download_denoised(channels=2)) == -1
        r.denoise()  # nine frames in eight chains: fine, and the context went on working through the refusals
        out = r.download_denoised()
        assert np.isfinite(out).all() and out.mean() > 0
        r.denoise(iterations=1, sigma_luminance=2.0)
        assert not np.array_equal(r.download_denoised(), out)
        r.reset()
        assert code(r.download_denoised) == -1  # reset: no result, no frames
        assert code(r.denoise) == -1
    with api.Renderer(s, flags=abi.FLAG_NO_AOV) as r:  # no guide layers: allowed, luminance-guided only
        r.render(0, 8)
        r.denoise()
        assert np.isfinite(r.download_denoised()).all()


def test_cli_writes_the_denoised_image(hip_lib, tmp_path):
    from PIL import Image
    p = tmp_path / "scene.pbrt"
    p.write_text(loader.scene_to_pbrt(scenes.cornell_box(96, 64)))

    def run(out, *extra):
        r = subprocess.run([CLI, str(p), "--spp", "16", "--out", str(tmp_path / out), "--aov-normal", str(tmp_path / ("n_" + out)),
                            "--aov-albedo", str(tmp_path / ("a_" + out)), *extra], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 0, r.stderr
        return r.stderr

    png = lambda name: np.asarray(Image.open(tmp_path / name).convert("RGB"))
    err = run("o.png", "--denoiser", "atrous")
    assert "INFO atrous denoiser:" in err and " ms" in err and "denoiser was enabled" not in err
    run("plain.png")
    with api.Renderer(loader.load_pbrt(str(p))) as rr:
        rr.render(0, 16)
        plain = api.to_rgb8(rr.download(0), 16)
        rr.denoise()
        want = api.to_rgb8(rr.download_denoised(), 16)
    assert np.array_equal(png("o.png"), want)
    assert np.array_equal(png("plain.png"), plain) and not np.array_equal(want, plain)
    assert np.array_equal(png("n_o.png"), png("n_plain.png")) and np.array_equal(png("a_o.png"), png("a_plain.png"))
