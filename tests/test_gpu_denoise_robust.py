"""GPU: firefly rejection inside the `atrous` denoiser (rene_denoise_robust, rene_denoise_tiles_robust) -- the two halves of its contract and the
rest of it: (a) with nothing trimmed it is the plain call bit for bit; (b) its trim counts are rene_resolve_robust's, capped so that two chains are
kept, bit for bit; against its specification, the numpy restatement of tests/atrous_robust_reference.py fed with the device's own frame chains;
the tiles call on an even context is the uniform call; what it buys on veach-mis; what it refuses.

BOUND: the restatement's fp32 run stays within 6.7e-7 (1 + |value|) of its fp64 run with the same decisions on oracle chains of the cases below
(tools/denoise_robust_study.py --spread: 4.7e-7 / 4.9e-7 cornell @ 12 at gain 1 / 0.35, 2.4e-7 / 3.8e-7 cornell @ 5, 6.4e-7 / 6.7e-7 veach @ 32,
3.9e-7 / 3.9e-7 the uneven schedule); 16 x that is 1.1e-5, below the 2e-5 of tests/test_gpu_denoise.py, which therefore stays."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import atrous_reference as ar
import atrous_robust_reference as arr
import atrous_tiles_reference as at
import test_gpu_denoise_tiles as tdt
from conftest import ROOT
from rene_amd import abi, api, loader, scenes

pytestmark = pytest.mark.gpu

BOUND = 2e-5
CASES = {
    "cornell-12": (lambda: scenes.cornell_box(100, 70), 12),  # ragged tiles, chains of 2 and 1 frames
    "cornell-5": (lambda: scenes.cornell_box(100, 70), 5),    # k = 5: three empty chains, the cap (k - 2) / 2 = 1 binds
    "veach-32": (lambda: scenes.veach_mis(96, 54), 32),       # fireflies everywhere
}
GAINS = (1.0, 0.35)


def rp(max_trim=3, gain=0.35):
    p = api.denoise_robust_params_default()
    p.max_trim, p.gain = max_trim, gain
    return p


def results(r):
    return tdt.results(r) + (r.download_denoised(abi.DENOISED_TRIM),)


def chain_count(frames):
    """k of a tile whose frames are 0 .. frames - 1."""
    return np.minimum(np.asarray(frames, np.int64), 8)


_jobs = {}


def job(name):
    """Computed once per case and left unchanged: the device's chains (every layer), and per gain the resolve's trim counts, the robust
    denoise's result and the restatement's in fp32 (its decisions) and fp64 (with them)."""
    if name in _jobs:
        return _jobs[name]
    make, spp = CASES[name]
    s = {"spp": spp}
    with api.Renderer(make()) as r:
        full = tdt.device_chain_layers(r, spp)
        s1, s2 = full[0, 1].copy(), full[0, 2].copy()
        for c in range(1, 8):
            s1 += full[c, 1]
            s2 += full[c, 2]
        film = (full[:, 0], at.chain_counts(0, spp), s1, s2)
        r.reset()
        r.render(0, spp)
        s["layers"] = [r.download(l) for l in range(3)]
        assert np.array_equal(s["layers"][1], s1) and np.array_equal(s["layers"][2], s2)  # the rebuilt chains are the job's
        for gain in GAINS:
            r.resolve_robust(max_trim=3, gain=gain)
            g = {"resolve_j": r.download_robust(abi.ROBUST_TRIM)}
            r.denoise(robust=rp(3, gain))
            g["got"] = results(r)
            r.denoise_tiles(robust=rp(3, gain))
            g["got_tiles"] = results(r)
            r32 = arr.denoise_robust(*film, gain=gain, dtype=np.float32)
            g["j32"] = r32["j"]
            g["want"] = arr.denoise_robust(*film, gain=gain, decisions=(r32["j"], r32["kept"]))
            s[gain] = g
        s["after"] = [r.download(l) for l in range(3)]
    _jobs[name] = s
    return s


def assert_within_bound(label, got, want, frames):
    radiance, var, mean = got[0][..., :3], got[1], got[2][..., :3]
    assert np.isfinite(radiance).all() and np.isfinite(var).all() and np.isfinite(mean).all()
    err = np.abs(mean.astype(np.float64) - want["mean"]) / (1 + np.abs(want["mean"]))
    y, x, ch = np.unravel_index(int(err.argmax()), err.shape)
    verr = np.abs(var.astype(np.float64) - want["var"]) - BOUND * np.abs(want["var"])
    rerr = np.abs(radiance.astype(np.float64) - want["radiance"]) / np.maximum(frames, 1)[..., None] / (1 + np.abs(want["mean"]))
    print(f"{label}: mean max err {err.max():.3g} of 1 + |value| at pixel ({x}, {y}) channel {ch} (device {mean[y, x, ch]:.6g}, restatement "
          f"{want['mean'][y, x, ch]:.6g}, j {want['j'][y, x]}); radiance / N {rerr.max():.3g}; variance max |diff| - rtol |v| = {verr.max():.3g} against atol "
          f"{BOUND * want['var'].max():.3g}; j > 0 on {float((want['j'] > 0).mean()):.3f} of the pixels (bound {BOUND:g})")
    assert err.max() <= BOUND, (label, float(err.max()), (int(x), int(y), int(ch)))
    assert rerr.max() <= BOUND, (label, float(rerr.max()))
    assert (verr <= BOUND * want["var"].max()).all(), (label, float(verr.max()))


# ---- (a) nothing trimmed: the plain call, bit for bit ------------------------------------------------------------------------------------------
def test_without_trimming_it_is_denoise_bit_for_bit():
    with api.Renderer(scenes.cornell_box(100, 70)) as r:
        r.render(0, 12)
        r.denoise()
        want = results(r)
        assert want[0].any() and want[1].any() and not want[3].any()  # DENOISED_TRIM after a plain call: zeros
        for gain in GAINS:
            r.denoise(robust=rp(0, gain))
            for a, b in zip(results(r), want):
                assert np.array_equal(a, b), gain
        # where trimming is allowed, the pixels it leaves alone start from the same record: the unfiltered variance plane says so
        r.denoise(robust=True)
        got = results(r)
        untouched = got[3] == 0
        assert untouched.any() and (~untouched).any() and np.array_equal(got[1][untouched], want[1][untouched])
        assert not np.array_equal(got[0], want[0])


def test_without_trimming_it_is_denoise_tiles_bit_for_bit_on_uneven_tiles():
    s = tdt.spec("cornell")  # cornell_box(161, 130): N_t = 0, 1, 11, 19, 35
    with api.Renderer(tdt.SPEC_CASES["cornell"]()) as r:
        at.run_schedule(r, s["classes"])
        assert np.array_equal(r.tile_frames(), s["tile_frames"]) and len(np.unique(s["tile_frames"])) == 5
        r.denoise_tiles()
        want = results(r)
        for a, b in zip(want[:3], s["got"]):
            assert np.array_equal(a, b)
        r.denoise_tiles(robust=rp(0, 1.0))
        for a, b in zip(results(r), want):
            assert np.array_equal(a, b)
        r.denoise_tiles(robust=True)
        got = results(r)
        untouched = got[3] == 0
        assert (~untouched).any() and np.array_equal(got[1][untouched], want[1][untouched])


# ---- (b) the trim counts: rene_resolve_robust's, capped ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("name", list(CASES))
def test_trim_counts_are_the_resolves_capped(name, gain):
    s = job(name)
    g = s[gain]
    k = int(chain_count(s["spp"]))
    want = np.minimum(g["resolve_j"], np.float32((k - 2) // 2))
    j = g["got"][3]
    print(f"{name}, gain {gain}: j histogram {np.bincount(j.astype(np.int64).ravel(), minlength=4).tolist()}, the resolve's "
          f"{np.bincount(g['resolve_j'].astype(np.int64).ravel(), minlength=4).tolist()}")
    assert j.dtype == np.float32 and np.array_equal(j, want)
    assert np.array_equal(j, g["j32"].astype(np.float32))  # ... and the fp32 restatement's
    if gain == 1.0:
        assert j.max() == (1 if name == "cornell-5" else 3)
        if name == "cornell-5":
            assert g["resolve_j"].max() == 2  # the cap binds
    elif name != "cornell-5":  # (k = 5 at gain 0.35: t = 0.875 G < 1, nothing is trimmed)
        assert 0 < (j > 0).mean() < 0.3


def test_trim_counts_on_uneven_tiles():
    s = tdt.spec("cornell")
    k = at.per_pixel(chain_count(s["tile_frames"]), 130, 161)
    with api.Renderer(tdt.SPEC_CASES["cornell"]()) as r:
        at.run_schedule(r, s["classes"])
        for gain in GAINS:
            r.resolve_robust(max_trim=3, gain=gain)
            want = np.minimum(r.download_robust(abi.ROBUST_TRIM), np.maximum((k - 2) // 2, 0).astype(np.float32))
            r.denoise_tiles(robust=rp(3, gain))
            j = r.download_denoised(abi.DENOISED_TRIM)
            assert np.array_equal(j, want) and (j > 0).any() and not j[k < 2].any()


def test_trim_counts_with_exact_ties_between_chains():
    """Crafted chains through rene_load_chains: every chain's sum at a pixel is one of three values, so most pixels hold ties, which the ranks
    break by chain index; some pixels hold one outlier, some are all zero (G = 0)."""
    h, w, n = 28, 40, 16
    rng = np.random.default_rng(7)
    level = rng.integers(0, 3, (8, h, w)).astype(np.float32) * 0.5
    level[rng.integers(0, 8, (h, w)), np.arange(h)[:, None], np.arange(w)[None, :]] *= np.where(rng.random((h, w)) < 0.2, 64.0, 1.0).astype(np.float32)
    level[:, :3, :5] = 0.0
    chains = np.zeros((8, 3, h, w, 3), np.float32)
    chains[:, 0] = level[..., None] * np.float32(n / 8)
    chains[:, 1] = np.array([0.0, 0.6, -0.8], np.float32) * np.float32(n / 8)
    chains[:, 2] = np.array([0.6, 0.5, 0.4], np.float32) * np.float32(n / 8)
    n_c = at.chain_counts(0, n)
    ties = (np.sort(level, axis=0)[1:] == np.sort(level, axis=0)[:-1]).any(0)
    with api.Renderer(scenes.cornell_box(w, h)) as r:
        r.load_chains(chains, 0, n)
        for gain in GAINS:
            r.resolve_robust(max_trim=3, gain=gain)
            resolve_j = r.download_robust(abi.ROBUST_TRIM)
            r.denoise(robust=rp(3, gain))
            got = results(r)
            j32, kept32 = arr.trim(chains[:, 0], n_c, 3, gain, np.float32)
            assert np.array_equal(got[3], np.minimum(resolve_j, np.float32(3))) and np.array_equal(got[3], j32.astype(np.float32))
            assert (ties & (j32 > 0)).sum() > 50 and not got[3][:3, :5].any()
            s1, s2 = chains[:, 1].sum(0), chains[:, 2].sum(0)
            want = arr.denoise_robust(chains[:, 0], n_c, s1, s2, gain=gain, decisions=(j32, kept32))
            assert_within_bound(f"ties, gain {gain}", got, want, np.full((h, w), n))


# ---- against the specification ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_specification(name, gain):
    s = job(name)
    g = s[gain]
    assert np.array_equal(g["got"][3], g["want"]["j"].astype(np.float32))  # the decisions are the device's, bit for bit
    assert_within_bound(f"{name}, gain {gain}", g["got"], g["want"], np.full(g["got"][1].shape, s["spp"]))
    assert np.array_equal(g["got"][0], g["got"][2] * np.float32(s["spp"]))  # the radiance is the mean times N, whatever was trimmed
    assert not g["got"][0][..., 3].any() and not g["got"][2][..., 3].any()


@pytest.mark.parametrize("gain", GAINS)
def test_device_equals_specification_on_uneven_tiles(gain):
    s = tdt.spec("cornell")
    chains, n_c, s1, s2 = s["film"]
    r32 = arr.denoise_robust(chains, n_c, s1, s2, gain=gain, dtype=np.float32)
    want = arr.denoise_robust(chains, n_c, s1, s2, gain=gain, decisions=(r32["j"], r32["kept"]))
    with api.Renderer(tdt.SPEC_CASES["cornell"]()) as r:
        at.run_schedule(r, s["classes"])
        r.denoise_tiles(robust=rp(3, gain))
        got = results(r)
        again = None
        if gain == GAINS[0]:  # deterministic, and the same from loaded chains
            r.reset()
            r.load_chains(s["loaded"], 0, 35, tile_frames=s["tile_frames"])
            r.denoise_tiles(robust=rp(3, gain))
            again = results(r)
    assert np.array_equal(got[3], want["j"].astype(np.float32)) and (got[3] > 0).any()
    valid = want["valid"]
    assert np.array_equal(valid, s["frames"] >= 2)
    assert_within_bound(f"uneven tiles, gain {gain}", got, want, s["frames"])
    assert np.array_equal(got[0][..., :3][~valid], s["layers"][0][~valid]) and np.array_equal(got[2][..., :3][~valid], s["plain_mean"][~valid])  # invalid: unfiltered
    assert np.array_equal(got[0][..., :3][valid], (got[2][..., :3] * s["frames"][..., None].astype(np.float32))[valid])
    for a, b in zip(again or (), got):
        assert np.array_equal(a, b)


# ---- even contexts: the tiles call is the uniform call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_even_context_the_tiles_call_equals_the_uniform_call(name):
    s = job(name)
    for gain in GAINS:
        for a, b in zip(s[gain]["got_tiles"], s[gain]["got"]):
            assert np.array_equal(a, b), (name, gain)
    for l in range(3):  # ... and none of the calls wrote the accumulation state
        assert np.array_equal(s["after"][l], s["layers"][l]), l


# ---- what it buys --------------------------------------------------------------------------------------------------------------------------
def test_quality_on_veach_mis():
    """relMSE(robust call) <= 0.25 relMSE(rene_denoise) on the same context, veach_mis(96, 54) @ 32 against 2048 device frames from frame 100000
    (the restatement on oracle chains measured 0.014 - 0.092 over the study's veach-mis rows)."""
    with api.Renderer(scenes.veach_mis(96, 54)) as r:
        r.render(100000, 2048)
        ref = r.download(0).astype(np.float64) / 2048
        r.reset()
        r.render(0, 32)
        noisy = r.download(0).astype(np.float64) / 32
        r.denoise()
        plain = r.download_denoised(abi.DENOISED_MEAN).astype(np.float64)
        r.denoise(robust=True)
        out = r.download_denoised(abi.DENOISED_MEAN).astype(np.float64)
        share = float((r.download_denoised(abi.DENOISED_TRIM) > 0).mean())
    e_noisy, e0, e1 = ar.relmse(noisy, ref), ar.relmse(plain, ref), ar.relmse(out, ref)
    print(f"veach_mis(96, 54) @ 32: relMSE plain mean {e_noisy:.4g}, rene_denoise {e0:.4g}, rene_denoise_robust {e1:.4g}, ratio {e1 / e0:.3f}; energy "
          f"(image mean over the reference's) {plain.mean() / ref.mean():.3f} and {out.mean() / ref.mean():.3f}; j > 0 on {share:.3f} of the pixels")
    assert e1 <= 0.25 * e0, (e0, e1)


# ---- what it refuses -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    sc = scenes.cornell_box(96, 64)
    classes = at.tile_classes(96, 64)

    def code(fn):
        with pytest.raises(api.ReneError) as e:
            fn()
        assert str(e.value).split(": ", 1)[1].strip()  # a message
        return e.value.code

    def skewed():
        p = rp()
        p.struct_size = 12
        return p

    with api.Renderer(sc, shard_mode=abi.SHARD_TILES, shard_rank=0, shard_count=2) as r:
        r.render(0, 8)
        assert code(lambda: r.denoise(robust=True)) == -4 and code(lambda: r.denoise_tiles(robust=True)) == -4  # RENE_ERR_UNSUPPORTED
        assert r.download(0).max() > 0
    with api.Renderer(sc, shard_mode=abi.SHARD_FRAMES, shard_rank=0, shard_count=2) as r:
        r.render(0, 8)
        assert code(lambda: r.denoise(robust=True)) == -4 and code(lambda: r.denoise_tiles(robust=True)) == -4
    with api.Renderer(sc) as r:
        for call in (r.denoise, r.denoise_tiles):
            assert code(lambda: call(robust=True)) == -1  # no frames
        r.render(0, 1)
        for call in (r.denoise, r.denoise_tiles):
            assert code(lambda: call(robust=True)) == -1  # one frame: k < 2
        assert code(lambda: r.download_denoised(abi.DENOISED_TRIM)) == -1  # nothing to download yet
        r.render(1, 15)
        before_image = [r.download(l) for l in range(3)]
        r.denoise(robust=True)
        before = results(r)
        assert (before[3] > 0).any()
        for call in (r.denoise, r.denoise_tiles):
            assert code(lambda: call(robust=rp(max_trim=4))) == -1
            assert code(lambda: call(robust=rp(gain=0.0))) == -1
            assert code(lambda: call(robust=rp(gain=float("nan")))) == -1
            assert code(lambda: call(robust=rp(gain=float("inf")))) == -1
            assert code(lambda: call(robust=skewed())) == -1
            assert code(lambda: call(robust=True, iterations=0)) == -1
            assert code(lambda: call(robust=True, sigma_luminance=float("nan"))) == -1
        with pytest.raises(TypeError):
            r.denoise(robust=0.35)
        assert code(lambda: r.download_denoised(what=7)) == -1
        buf = np.zeros(96 * 64 * 3, np.float32)  # (the Python call fixes a plane's channels itself)
        assert api.lib().rene_download_denoised(r._h, abi.DENOISED_TRIM, 3, buf.ctypes.data_as(C.c_void_p), buf.size) == -1 and not buf.any()
        for a, b in zip(results(r), before):  # a refusal leaves the previous result downloadable
            assert np.array_equal(a, b)
        for l in range(3):  # ... and the accumulation state is what it was
            assert np.array_equal(r.download(l), before_image[l]), l
        ptr, n = r.denoised_buffer()
        assert ptr and n == 96 * 64 * 4
        r.denoise()  # a plain call after a robust one: the trim counts it serves are zeros
        assert not r.download_denoised(abi.DENOISED_TRIM).any()
        r.reset()
        assert code(lambda: r.download_denoised(abi.DENOISED_TRIM)) == -1  # reset: no result
        at.run_schedule(r, classes)  # uneven tiles: the uniform call refuses, the tiles call does not
        r.denoise_tiles(robust=True)
        kept = results(r)
        assert code(lambda: r.denoise(robust=True)) == -4
        for a, b in zip(results(r), kept):
            assert np.array_equal(a, b)
    with api.Renderer(sc) as r:  # an exchange consumes the chains
        r.comm_init(1, 0, api.comm_unique_id())
        r.render(0, 16)
        r.gather_tiles(0)
        assert code(lambda: r.denoise(robust=True)) == -4 and code(lambda: r.denoise_tiles(robust=True)) == -4


def test_cli_writes_the_image_of_the_robust_call(tmp_path):
    from PIL import Image
    cli = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
    p = tmp_path / "scene.pbrt"
    p.write_text(loader.scene_to_pbrt(scenes.cornell_box(96, 64)))

    def run(out, *extra):
        r = subprocess.run([cli, str(p), "--out", str(tmp_path / out), "--spp", "16", *extra], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 0, r.stderr
        return r.stderr

    png = lambda name: np.asarray(Image.open(tmp_path / name).convert("RGB"))
    err = run("r.png", "--denoiser", "atrous", "--reject-fireflies")
    m = re.search(r"INFO firefly rejection: ([0-9.]+) % of the pixels left chains out \(max_trim 3, gain 0.35\)", err)
    assert m and "INFO atrous denoiser:" in err, err
    run("t.png", "--denoiser", "atrous-tiles", "--reject-gain", "0.35")  # a parameter alone asks for the rejection
    assert (tmp_path / "t.png").read_bytes() == (tmp_path / "r.png").read_bytes()
    run("zero.png", "--denoiser", "atrous", "--reject-max-trim", "0")
    run("plain.png", "--denoiser", "atrous")
    assert (tmp_path / "zero.png").read_bytes() == (tmp_path / "plain.png").read_bytes()
    with api.Renderer(loader.load_pbrt(str(p))) as rr:
        rr.render(0, 16)
        rr.denoise(robust=True)
        want = api.to_rgb8(rr.download_denoised(), 16)
        share = 100.0 * float((rr.download_denoised(abi.DENOISED_TRIM) > 0).mean())
    assert np.array_equal(png("r.png"), want) and not np.array_equal(png("plain.png"), want)
    assert abs(float(m.group(1)) - share) <= 0.006 and share > 0
