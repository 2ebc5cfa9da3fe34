"""GPU: the noise estimate (rene_estimate_noise) against its specification -- the numpy restatement of tests/noise_reference.py fed with the
device's own frame chains, rebuilt through the public ABI -- and its contract: read-only, deterministic, independent of how a job is cut into
calls and into tile shards, refusing what it cannot do; rendering to a noise target; and the command line."""
import os
import re
import subprocess

import numpy as np
import pytest

import noise_reference as nr
from conftest import ROOT
from rene_amd import abi, api, loader, scenes

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
# 16 x the largest fp32-vs-fp64 spread of the restatement itself, 8.2e-8, measured on the CPU oracle's chains of the five cases below as
# max over tiles of |fp32 - fp64| / (|fp64| + the largest tile's value): sum_var 7.2e-9 cornell, 6.1e-8 zoo, 4.4e-8 fog, 4.6e-8 dragon,
# 5.1e-8 cornell 1283x821; sum_lum 2.6e-8, 7.4e-9, 2.3e-8, 2.3e-8, 8.2e-8.  (Not tuned on the device's output.)
BOUND = 16 * 8.2e-8


def device_chains(r, spp):
    """The chains a job of frames 0 .. spp - 1 leaves on the device: for chain c, reset, render every frame f = c (mod 8) on its own, download
    -- the other chains hold 0 and adding 0 is exact, so the download IS C_c bit for bit (the trick of tests/test_gpu_denoise.py)."""
    chains = np.zeros((8, r.yres, r.xres, 3), np.float32)
    n_c = np.zeros(8)
    for c in range(8):
        r.reset()
        for f in range(c, spp, 8):
            r.render(f, 1)
            n_c[c] += 1
        chains[c] = r.download(0)
    return chains, n_c


def tiles_as_arrays(t):
    return t["sum_var"].astype(np.float64), t["sum_lum"].astype(np.float64), t["n_pixels"].astype(np.int64)


def check_against_restatement(r, spp, label):
    chains, n_c = device_chains(r, spp)
    r.reset()
    r.render(0, spp)
    s0 = r.download(0)
    acc = chains[0].copy()
    for c in range(1, 8):
        acc += chains[c]
    assert np.array_equal(acc, s0), label  # the rebuilt chains are the job's chains
    est = r.estimate_noise()
    a, b, n = tiles_as_arrays(r.noise_tiles())
    want = nr.estimate(chains, n_c, floor=est.luminance_floor)
    w32 = nr.estimate(chains, n_c, floor=est.luminance_floor, dtype=np.float32)
    assert np.array_equal(n, want["n"]), label  # exact
    assert est.n_pixels == r.xres * r.yres and est.n_tiles == n.size and est.n_frames == spp and est.n_chains == int((n_c > 0).sum())
    scale_a, scale_b = want["A"].max(), want["B"].max()
    err_a = np.abs(a - want["A"]) / (np.abs(want["A"]) + scale_a)
    err_b = np.abs(b - want["B"]) / (np.abs(want["B"]) + scale_b)
    spread_a = np.abs(w32["A"] - want["A"]) / (np.abs(want["A"]) + scale_a)
    spread_b = np.abs(w32["B"] - want["B"]) / (np.abs(want["B"]) + scale_b)
    print(f"{label}: sum_var max err {err_a.max():.3g}, sum_lum max err {err_b.max():.3g} of |value| + largest tile (bound {BOUND:.3g}; the restatement's own "
          f"fp32 spread on these chains {spread_a.max():.3g} / {spread_b.max():.3g}); noise {est.noise:.5f} (restatement {want['noise']:.5f}), "
          f"rel_rmse {est.rel_rmse:.5f}, worst tile {est.worst_tile_noise:.5f} at {est.worst_tile}")
    assert np.isfinite(a).all() and np.isfinite(b).all() and (a >= 0).all()
    assert err_a.max() <= BOUND, (label, float(err_a.max()))
    assert err_b.max() <= BOUND, (label, float(err_b.max()))
    # the image figures follow from the tile records by the definition, in fp64
    fig = nr.figures(a, b, n, est.luminance_floor)
    for k in ("sum_var", "sum_lum", "sum_weighted_q", "noise", "rel_rmse", "worst_tile_noise"):
        assert abs(getattr(est, k) - fig[k]) <= 1e-12 * abs(fig[k]), (label, k)
    assert est.worst_tile == fig["worst_tile"]


SPEC_CASES = {
    "cornell": (lambda: scenes.cornell_box(100, 70), 12),       # ragged tiles, chains of 2 and 1 frames
    "zoo": (lambda: scenes.material_zoo(192, 128), 32),         # textures, environment map, every material
    "fog": (lambda: scenes.cornell_fog(96, 64), 32),            # volpath
    "dragon": (lambda: scenes.dragon_class(240, 136), 16),      # BVH traversal-restart kernel
    "cornell-1283x821": (lambda: scenes.cornell_box(1283, 821), 8),  # more than 2^20 pixels, neither side a multiple of 32
}


@pytest.mark.parametrize("name", list(SPEC_CASES))
def test_device_equals_specification(name):
    make, spp = SPEC_CASES[name]
    with api.Renderer(make()) as r:
        check_against_restatement(r, spp, name)


def raw(t):
    """The records' bits: [ty][tx][4] u32."""
    return np.ascontiguousarray(t).view(np.uint32).reshape(t.shape + (4,))


def test_read_only_and_deterministic():
    s = scenes.cornell_box(100, 70)
    with api.Renderer(s) as r, api.Renderer(s) as plain:
        r.render(0, 12)
        plain.render(0, 12)
        before = [r.download(l) for l in range(3)]
        e1 = r.estimate_noise()
        t1 = r.noise_tiles()
        for l in range(3):
            assert np.array_equal(r.download(l), before[l]) and np.array_equal(plain.download(l), before[l])
        e2 = r.estimate_noise()
        assert np.array_equal(raw(r.noise_tiles()), raw(t1))  # bit-equal records
        assert e1.as_dict() == e2.as_dict()
        assert t1.shape == (3, 4) and (t1["n_pixels"] > 0).all() and (t1["reserved"] == 0).all() and e1.noise > 0
        r.render(12, 8)  # later frames are what they are without the call
        plain.render(12, 8)
        for l in range(3):
            assert np.array_equal(r.download(l), plain.download(l))
        assert r.estimate_noise().as_dict() == plain.estimate_noise().as_dict()
        assert r.estimate_noise(luminance_floor=0.5).noise < r.estimate_noise().noise  # the floor is a parameter
        assert np.array_equal(raw(r.noise_tiles()), raw(plain.noise_tiles()))          # ... of the figures, not of the records


def test_independent_of_the_cut():
    s = scenes.cornell_box(100, 70)
    with api.Renderer(s) as a, api.Renderer(s) as b:
        a.render(0, 24)
        for first in (0, 8, 16):
            b.render(first, 8)
        ea, eb = a.estimate_noise(), b.estimate_noise()
        assert np.array_equal(raw(a.noise_tiles()), raw(b.noise_tiles()))
        assert ea.as_dict() == eb.as_dict()


def test_tile_shards_report_their_tiles_and_add_up():
    s = scenes.material_zoo(203, 77)  # 7 x 3 tiles, ragged on both sides
    with api.Renderer(s) as whole, api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=0, shard_count=2) as s0, \
            api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=1, shard_count=2) as s1:
        for r in (whole, s0, s1):
            r.render(0, 24)
        ew, tw = whole.estimate_noise(), whole.noise_tiles()
        parts = []
        owner = np.arange(tw.size).reshape(tw.shape) % 2
        for rank, r in enumerate((s0, s1)):
            parts.append(r.estimate_noise())
            t = r.noise_tiles()
            assert t.shape == tw.shape
            assert np.array_equal(raw(t)[owner == rank], raw(tw)[owner == rank])  # owned tiles: bit-identical to the unsharded context's
            assert (raw(t)[owner != rank] == 0).all()                              # the others: zero
            assert parts[-1].n_tiles == int((owner == rank).sum()) and parts[-1].n_pixels == int(tw["n_pixels"][owner == rank].sum())
        both = api.noise_combine(parts)
        assert both.n_tiles == ew.n_tiles and both.n_pixels == ew.n_pixels == 203 * 77 and both.n_frames == 24 and both.n_chains == 8
        assert both.worst_tile == ew.worst_tile and both.luminance_floor == ew.luminance_floor
        for k in ("sum_var", "sum_lum", "sum_weighted_q", "noise", "rel_rmse", "worst_tile_noise"):
            assert abs(getattr(both, k) - getattr(ew, k)) <= 1e-12 * abs(getattr(ew, k)), k
        assert both.noise > 0


def test_refusals_leave_the_context_usable():
    s = scenes.cornell_box(64, 48)

    def code(fn):
        with pytest.raises(api.ReneError) as e:
            fn()
        assert str(e.value).split(": ", 1)[1].strip()  # a message
        return e.value.code

    with api.Renderer(s) as r:
        assert code(r.estimate_noise) == -1   # no frames
        assert code(r.noise_tiles) == -1      # no estimate yet
        r.render(0, 1)
        assert code(r.estimate_noise) == -1   # one frame: one chain
        r.render(8, 1)
        assert code(r.estimate_noise) == -1   # two frames, both in chain 0
        r.render(1, 7)
        assert code(lambda: r.estimate_noise(luminance_floor=0.0)) == -1
        assert code(lambda: r.estimate_noise(luminance_floor=-0.01)) == -1
        assert code(lambda: r.estimate_noise(luminance_floor=float("nan"))) == -1
        assert code(lambda: r.estimate_noise(luminance_floor=float("inf"))) == -1
        p = api.noise_params_default()
        p.struct_size = 12
        out = abi.NoiseEstimate()
        import ctypes as C
        assert api.lib().rene_estimate_noise(r._h, C.byref(p), C.byref(out)) == -1 and b"struct_size" in api.lib().rene_last_error()
        assert code(r.noise_tiles) == -1      # still none
        est = r.estimate_noise()              # nine frames in eight chains: fine, and the context went on working through the refusals
        assert est.n_frames == 9 and est.n_chains == 8 and np.isfinite(est.noise) and est.noise > 0
        small = (abi.NoiseTile * 3)()
        assert api.lib().rene_download_noise_tiles(r._h, small, 3) == -1  # the grid is 2 x 2
        assert r.noise_tiles().shape == (2, 2)
        r.reset()
        assert code(r.noise_tiles) == -1      # reset: no estimate, no frames
        assert code(r.estimate_noise) == -1
        # an exchange consumes the chains
        r.comm_init(1, 0, api.comm_unique_id())
        r.render(0, 16)
        assert r.estimate_noise().n_frames == 16
        r.gather_tiles(0)
        assert code(r.estimate_noise) == -4   # RENE_ERR_UNSUPPORTED, until the reset
        r.reset()
        r.render(0, 16)
        assert r.estimate_noise().n_frames == 16
    with api.Renderer(s, shard_mode=abi.SHARD_FRAMES, shard_rank=0, shard_count=2) as r:
        r.render(0, 32)
        assert code(r.estimate_noise) == -4   # a frame shard holds a share of every pixel's frames
        assert r.download(0).max() > 0
    with api.Renderer(s, shard_mode=abi.SHARD_FRAMES, shard_rank=0, shard_count=1) as r:  # shard_count 1 is unsharded, whatever the mode
        r.render(0, 16)
        assert r.estimate_noise().n_pixels == 64 * 48


def test_render_until():
    s = scenes.cornell_box(100, 70)
    with api.Renderer(s) as r, api.Renderer(s) as fresh:
        with api.Renderer(s) as probe:
            probe.render(0, 64)
            at64 = probe.estimate_noise().noise
        target = 0.6 * at64  # needs about 64 / 0.36 = 180 frames
        n, est = r.render_until(target, 4096, batch=64)
        print(f"render_until: noise {at64:.4f} at 64 frames, target {target:.4f} met with {est.noise:.4f} after {n} frames")
        assert 64 < n < 4096 and n % 8 == 0 and est.noise <= target and est.n_frames == n
        fresh.render(0, n)
        for l in range(3):
            assert np.array_equal(r.download(l), fresh.download(l))  # bit for bit the image of one render(0, n)
        assert fresh.estimate_noise().as_dict() == est.as_dict()
        # an unreachable target stops exactly at the cap, also where the cap is no multiple of 8
        r.reset()
        n, est = r.render_until(1e-9, 100, batch=16)
        assert n == 100 and est.n_frames == 100 and est.noise > 1e-9
        fresh.reset()
        fresh.render(0, 100)
        assert np.array_equal(r.download(0), fresh.download(0))
        # a lenient one stops after the first batch; frames from first_frame on
        r.reset()
        n, est = r.render_until(1e3, 4096, batch=32, first_frame=40)
        assert n == 32 and est.n_frames == 32
        fresh.reset()
        fresh.render(40, 32)
        assert np.array_equal(r.download(0), fresh.download(0))
        for bad in (dict(batch=8), dict(batch=20)):
            with pytest.raises(ValueError):
                r.render_until(0.1, 64, **bad)


def test_noise_halves_for_four_times_the_frames():
    """cornell_fog(64, 64), 16 against 64 frames: the band of tests/noise_reference.py (2 +- 0.25, from the oracle's eight seeds)."""
    with api.Renderer(scenes.cornell_fog(64, 64)) as r:
        r.render(0, 16)
        n16 = r.estimate_noise().noise
        r.render(16, 48)
        n64 = r.estimate_noise().noise
    print(f"fog: noise {n16:.4f} at 16 frames, {n64:.4f} at 64, ratio {n16 / n64:.3f}")
    assert abs(n16 / n64 - 2) <= nr.LAW_BANDS["fog"][0], (n16, n64)


def test_cli_target_noise_and_noise_map(hip_lib, tmp_path):
    from PIL import Image
    p = tmp_path / "scene.pbrt"
    p.write_text(loader.scene_to_pbrt(scenes.cornell_box(96, 64)))

    def run(out, *extra):
        r = subprocess.run([CLI, str(p), "--out", str(tmp_path / out), *extra], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 0, r.stderr
        return r.stderr

    png = lambda name: np.asarray(Image.open(tmp_path / name))
    with api.Renderer(loader.load_pbrt(str(p))) as rr:
        rr.render(0, 32)
        at32 = rr.estimate_noise().noise
        # a lenient target: ends below the cap
        target = 0.7 * at32  # about 32 / 0.49 = 65 frames
        err = run("t.png", "--spp", "2048", "--batch", "32", "--target-noise", repr(target), "--noise-map", str(tmp_path / "m.png"))
        last = err.strip().splitlines()[-1]
        m = re.fullmatch(r"noise: (\S+) \(worst tile (\S+) at (\d+),(\d+)\) after (\d+) samples", last)
        assert m, err
        n = int(m.group(5))
        assert 32 < n < 2048 and float(m.group(1)) <= target and f"Samples: {n} / 2048" in err
        rr.reset()
        n_api, est = rr.render_until(target, 2048, batch=32)
        assert n_api == n  # the same schedule
        assert float(m.group(1)) == pytest.approx(est.noise, rel=1e-5) and float(m.group(2)) == pytest.approx(est.worst_tile_noise, rel=1e-5)
        assert (int(m.group(3)), int(m.group(4))) == (est.worst_tile % 3, est.worst_tile // 3)
        assert np.array_equal(png("t.png"), api.to_rgb8(rr.download(0), n))  # the image of the frames it stopped at
        tiles = rr.noise_tiles()
        tn = nr.figures(*[tiles[k].astype(np.float64) for k in ("sum_var", "sum_lum", "n_pixels")], est.luminance_floor)["tile_noise"]
        grey = png("m.png")
        assert grey.shape == (2, 3) and grey.dtype == np.uint8  # tiles_x x tiles_y, 8-bit grey
        assert np.abs(grey.astype(int) - np.round(255 * np.minimum(1, tn / target)).astype(int)).max() <= 1
        # the map alone: a fixed --spp, scaled by the worst tile
        err = run("f.png", "--spp", "32", "--batch", "32", "--noise-map", str(tmp_path / "m2.png"))
        m = re.fullmatch(r"noise: (\S+) \(worst tile (\S+) at (\d+),(\d+)\) after 32 samples", err.strip().splitlines()[-1])
        assert m and float(m.group(1)) == pytest.approx(at32, rel=1e-5), err
        grey = png("m2.png")
        assert grey.shape == (2, 3) and grey.max() == 255 and grey[int(m.group(4)), int(m.group(3))] == 255
        # --denoiser atrous denoises the frames the target stopped at
        err = run("d.png", "--spp", "2048", "--batch", "32", "--target-noise", repr(target), "--denoiser", "atrous")
        assert f"after {n} samples" in err.strip().splitlines()[-1] and "INFO atrous denoiser:" in err
        rr.denoise()
        assert np.array_equal(png("d.png"), api.to_rgb8(rr.download_denoised(), n))
        # a run without the flags is what it was: the image of --spp frames, no noise line
        err = run("plain.png", "--spp", "32", "--batch", "32")
        assert "noise:" not in err and err.strip().splitlines()[-1].startswith("INFO End")
        rr.reset()
        rr.render(0, 32)
        assert np.array_equal(png("plain.png"), api.to_rgb8(rr.download(0), 32)) and np.array_equal(png("plain.png"), png("f.png"))
        assert not (tmp_path / "noise.png").exists()
    r = subprocess.run([CLI, str(p), "--target-noise", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--target-noise" in r.stderr
