"""GPU: the firefly-robust resolve (rene_resolve_robust) against its specification -- the numpy restatement of tests/robust_reference.py in
np.float32, fed with the device's own frame chains rebuilt through the public ABI, BIT FOR BIT on the image and on the trim plane -- and its
contract: where nothing is trimmed it is rene_download_mean; read-only, deterministic, independent of how a job is cut into calls and into
tile shards; uneven tiles resolved as shorter uniform jobs; refusing what it cannot do; the error it removes; and the command line."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_reference as ar
import robust_reference as rr
from atrous_reference import relmse
from conftest import GOLDEN, ROOT
from rene_amd import abi, api, loader, scenes

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
# The tile sums: the device adds a tile's pixels in its own fixed order (four slots, a wave butterfly, four wave partials), the restatement in
# numpy's.  The pixels themselves are held bit for bit, so the sums are compared with the restatement's fp32 pixels summed in fp64, and the bound
# is 16 x the restatement's own fp32-vs-fp64 spread, measured on the CPU oracle's chains of the five scenes below (tools/robust_bias.py --spread)
# as max over tiles of |fp32 - fp64| / (|fp64| + the largest tile's value):
#   sum_lum_plain   2.6e-8 cornell @ 12, 6.7e-9 cornell @ 5, 2.3e-8 fog, 2.6e-8 veach, 2.3e-8 dragon
#   sum_lum_robust  2.9e-8, (6.6e-3), 9.0e-9, 3.3e-8, 3.8e-8
#   the fp32 run's own pixels summed in fp32 against the same pixels summed in fp64: 2.9e-8 / 3.0e-8, 6.5e-9 / 3.2e-8, 2.1e-8 / 8.7e-9,
#   4.1e-8 / 4.8e-8, 2.1e-8 / 3.8e-8
# The figure in brackets is no rounding spread: at five frames 162 of 7000 pixels sit exactly on a threshold of step 4 (one bright chain of
# five: G = 4/5, t = 2 to the last bit) and get another j in fp64 than in fp32.  It is left out -- the device is held to the fp32 pixels -- and
# the largest of the others, 4.8e-8, is taken.  (Not tuned on the device's output.)
BOUND = 16 * 4.8e-8


def device_chains(r, spp, first=0):
    """The chains a job of frames first .. first + spp - 1 leaves on the device: for chain c, reset, render every frame f = c (mod 8) on its
    own, download -- the other chains hold 0 and adding 0 is exact, so the download IS C_c bit for bit (the trick of tests/test_gpu_noise.py)."""
    chains = np.zeros((8, r.yres, r.xres, 3), np.float32)
    for c in range(8):
        r.reset()
        for f in range(first, first + spp):
            if f % 8 == c:
                r.render(f, 1)
        chains[c] = r.download(0)
    return chains, rr.chain_counts(spp, first)


def raw(t):
    """The records' bits: [ty][tx][4] u32."""
    return np.ascontiguousarray(t).view(np.uint32).reshape(t.shape + (4,))


def check_against_restatement(r, spp, label, **params):
    chains, n_c = device_chains(r, spp)
    r.reset()
    r.render(0, spp)
    s0 = r.download(0)
    acc = chains[0].copy()
    for c in range(1, 8):
        acc += chains[c]
    assert np.array_equal(acc, s0), label  # the rebuilt chains are the job's chains
    summ = r.resolve_robust(**params)
    img, img4, j, tiles = r.download_robust(), r.download_robust(channels=4), r.download_robust(abi.ROBUST_TRIM), r.robust_tiles()
    want = rr.resolve(chains, n_c, dtype=np.float32, **params)
    assert want["image"].dtype == np.float32 and img.dtype == np.float32 and j.shape == (r.yres, r.xres)
    diff = (img != want["image"]).any(axis=-1)
    print(f"{label}: {int(diff.sum())} of {diff.size} pixels differ from the restatement, {int((j != want['j']).sum())} in j; "
          f"j histogram {np.bincount(want['j'].ravel(), minlength=4).tolist()}, kept energy {summ.kept_energy:.4f}")
    assert np.array_equal(j, want["j"].astype(np.float32)), label          # bit for bit: no tolerance
    assert np.array_equal(img, want["image"]), label
    assert np.array_equal(img4[..., :3], img) and not img4[..., 3].any()  # alpha 0
    a, b, n, nt = rr.tile_records(want["lum_plain"].astype(np.float64), want["lum_robust"].astype(np.float64), want["j"])
    assert np.array_equal(tiles["n_pixels"], n) and np.array_equal(tiles["n_trimmed"], nt), label  # exact
    err_a = np.abs(tiles["sum_lum_plain"] - a) / (np.abs(a) + a.max())
    err_b = np.abs(tiles["sum_lum_robust"] - b) / (np.abs(b) + b.max())
    print(f"{label}: sum_lum_plain max err {err_a.max():.3g}, sum_lum_robust max err {err_b.max():.3g} of |value| + largest tile (bound {BOUND:.3g})")
    assert err_a.max() <= BOUND and err_b.max() <= BOUND, (label, float(err_a.max()), float(err_b.max()))
    # the summary follows from the tile records by the definition, in fp64 and in tile order
    fig = rr.summary(tiles["sum_lum_plain"], tiles["sum_lum_robust"], tiles["n_pixels"], tiles["n_trimmed"])
    assert (summ.n_tiles, summ.n_pixels, summ.n_trimmed) == (fig["n_tiles"], fig["n_pixels"], fig["n_trimmed"]) == (n.size, r.xres * r.yres, int((want["j"] > 0).sum()))
    assert summ.sum_lum_plain == fig["sum_lum_plain"] and summ.sum_lum_robust == fig["sum_lum_robust"] and summ.kept_energy == fig["kept_energy"]
    assert summ.n_frames == spp and summ.struct_size == 64
    return want, chains, n_c


SPEC_CASES = {
    "cornell": (lambda: scenes.cornell_box(100, 70), 12, 0),        # ragged tiles, chains of 2 and 1 frames
    "cornell-5": (lambda: scenes.cornell_box(100, 70), 5, 0),       # k = 5: three empty chains, j capped at 2
    "fog": (lambda: scenes.cornell_fog(96, 64), 32, 0),             # volpath
    "veach": (lambda: scenes.veach_mis(96, 54), 32, 0),             # fireflies everywhere
    "dragon": (lambda: scenes.dragon_class(240, 136), 16, 0),       # BVH traversal-restart kernel
    "dragon-wavefront": (lambda: scenes.dragon_class(240, 136), 16, abi.FLAG_WAVEFRONT),  # the stage-separated integrator: chains all the same
}


@pytest.mark.parametrize("name", list(SPEC_CASES))
def test_device_equals_specification_bit_for_bit(name):
    make, spp, flags = SPEC_CASES[name]
    with api.Renderer(make(), flags=flags) as r:
        want, chains, n_c = check_against_restatement(r, spp, name)
        assert (want["j"] > 0).any()  # the comparison is not of one plain mean with another
        if name == "cornell-5":
            assert want["j"].max() <= 2
        if name == "cornell":  # the parameters reach the device
            for params in (dict(max_trim=1), dict(gain=0.5), dict(max_trim=2, gain=3.0)):
                w = rr.resolve(chains, n_c, dtype=np.float32, **params)
                s = r.resolve_robust(**params)
                assert np.array_equal(r.download_robust(), w["image"]) and np.array_equal(r.download_robust(abi.ROBUST_TRIM), w["j"].astype(np.float32)), params
                assert s.max_trim == params.get("max_trim", 3) and s.gain == np.float32(params.get("gain", 1.0))


def test_untrimmed_pixels_are_download_mean():
    with api.Renderer(scenes.cornell_box(100, 70)) as r:
        r.render(0, 12)
        mean = r.download_mean(0)
        s = r.resolve_robust()
        img, j = r.download_robust(), r.download_robust(abi.ROBUST_TRIM)
        assert (j == 0).any() and (j > 0).any() and 0 < s.kept_energy < 1
        assert np.array_equal(img[j == 0], mean[j == 0])      # bit for bit
        assert (img[j > 0] != mean[j > 0]).any()
        s0 = r.resolve_robust(max_trim=0)
        assert np.array_equal(r.download_robust(), mean) and not r.download_robust(abi.ROBUST_TRIM).any()
        assert s0.kept_energy == 1.0 and s0.n_trimmed == 0 and s0.sum_lum_plain == s0.sum_lum_robust > 0
        t = r.robust_tiles()
        assert np.array_equal(t["sum_lum_plain"], t["sum_lum_robust"]) and not t["n_trimmed"].any()


def test_read_only_deterministic_and_independent_of_the_cut():
    s = scenes.cornell_box(100, 70)
    with api.Renderer(s) as r, api.Renderer(s) as plain, api.Renderer(s) as cut:
        r.render(0, 32)
        plain.render(0, 32)
        for first, n in ((0, 5), (5, 20), (25, 7)):
            cut.render(first, n)
        before = [r.download(l) for l in range(3)]
        s1 = r.resolve_robust()
        i1, j1, t1 = r.download_robust(), r.download_robust(abi.ROBUST_TRIM), r.robust_tiles()
        for l in range(3):
            assert np.array_equal(r.download(l), before[l]) and np.array_equal(plain.download(l), before[l])
        s2 = r.resolve_robust()
        assert np.array_equal(r.download_robust(), i1) and np.array_equal(r.download_robust(abi.ROBUST_TRIM), j1) and np.array_equal(raw(r.robust_tiles()), raw(t1))
        assert s1.as_dict() == s2.as_dict() and t1.shape == (3, 4) and (t1["n_pixels"] > 0).all()
        sc = cut.resolve_robust()
        assert np.array_equal(cut.download_robust(), i1) and np.array_equal(cut.download_robust(abi.ROBUST_TRIM), j1) and np.array_equal(raw(cut.robust_tiles()), raw(t1))
        assert sc.as_dict() == s1.as_dict()
        r.render(32, 8)  # later frames are what they are without the call
        plain.render(32, 8)
        for l in range(3):
            assert np.array_equal(r.download(l), plain.download(l))
        assert r.resolve_robust().as_dict() == plain.resolve_robust().as_dict()
        assert np.array_equal(r.download_robust(), plain.download_robust())
        assert r.estimate_noise().as_dict() == plain.estimate_noise().as_dict()


def test_tile_shards_resolve_their_tiles_and_add_up():
    s = scenes.cornell_box(100, 70)  # 4 x 3 tiles, ragged on both sides
    with api.Renderer(s) as whole, api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=0, shard_count=2) as s0, \
            api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=1, shard_count=2) as s1:
        for r in (whole, s0, s1):
            r.render(0, 12)
        sw, iw, jw, tw = whole.resolve_robust(), whole.download_robust(), whole.download_robust(abi.ROBUST_TRIM), whole.robust_tiles()
        owner = np.arange(tw.size).reshape(tw.shape) % 2
        owner_px = np.zeros((70, 100), int)
        for t, sl in ar.tile_slices(100, 70):
            owner_px[sl] = owner[t]
        parts = []
        for rank, r in enumerate((s0, s1)):
            parts.append(r.resolve_robust())
            img, j, t = r.download_robust(), r.download_robust(abi.ROBUST_TRIM), r.robust_tiles()
            mine = owner_px == rank
            assert np.array_equal(img[mine], iw[mine]) and np.array_equal(j[mine], jw[mine])  # owned tiles: the unsharded context's bits
            assert not img[~mine].any() and not j[~mine].any()                               # the others: zero
            assert np.array_equal(raw(t)[owner == rank], raw(tw)[owner == rank]) and not raw(t)[owner != rank].any()
            assert parts[-1].n_tiles == int((owner == rank).sum()) and parts[-1].n_pixels == int(tw["n_pixels"][owner == rank].sum())
        both = api.robust_combine(parts)
        assert (both.n_tiles, both.n_pixels, both.n_trimmed, both.n_frames) == (sw.n_tiles, sw.n_pixels, sw.n_trimmed, 12) and sw.n_pixels == 7000
        for k in ("sum_lum_plain", "sum_lum_robust", "kept_energy"):
            assert abs(getattr(both, k) - getattr(sw, k)) <= 1e-12 * abs(getattr(sw, k)), k


def _uniform_resolves(make, counts):
    out = {}
    with api.Renderer(make()) as r:
        for n in counts:
            r.reset()
            r.render(0, n)
            r.resolve_robust()
            out[n] = (r.download_robust(), r.download_robust(abi.ROBUST_TRIM), r.robust_tiles())
    return out


def _assert_tiles_are_uniform_jobs(r, frames, ref):
    """Every tile's image, j and record are those of the uniform context after render(0, N_t): frames [ty][tx]."""
    img, j, tiles = r.download_robust(), r.download_robust(abi.ROBUST_TRIM), r.robust_tiles()
    for t, sl in ar.tile_slices(r.xres, r.yres):
        n = int(frames[t])
        if n == 0:
            assert not img[sl].any() and not j[sl].any()
            assert tiles["n_pixels"][t] == ar.tile_pixels(r.xres, r.yres)[t] and not raw(tiles)[t][[0, 1, 3]].any()
            continue
        assert np.array_equal(img[sl], ref[n][0][sl]) and np.array_equal(j[sl], ref[n][1][sl]), (t, n)
        assert np.array_equal(raw(tiles)[t], raw(ref[n][2])[t]), (t, n)
    return img, j, tiles


def test_uneven_tiles_are_shorter_uniform_jobs():
    """The 96 x 64 class layout of tests/test_gpu_adaptive.py: class A stopped at 16 frames, the rest at 24; then that file's own schedule (class A
    never rendered, 11, 19 and 35 frames: chains of unequal length, and a tile without frames)."""
    make = lambda: scenes.cornell_box(96, 64)
    classes = ar.tile_classes(96, 64)
    ref = _uniform_resolves(make, (16, 24, 11, 19, 35))
    with api.Renderer(make()) as r:
        r.render(0, 16)
        r.set_active_tiles(classes != "A")
        r.render(16, 8)
        frames = np.where(classes == "A", 16, 24)
        assert np.array_equal(r.tile_frames(), frames)
        s = r.resolve_robust()
        img, j, tiles = _assert_tiles_are_uniform_jobs(r, frames, ref)
        assert s.n_frames == 24 and s.n_pixels == 96 * 64 and s.n_tiles == 6 and s.n_trimmed == int((j > 0).sum()) > 0
        assert s.sum_lum_robust == rr.summary(tiles["sum_lum_plain"], tiles["sum_lum_robust"], tiles["n_pixels"], tiles["n_trimmed"])["sum_lum_robust"]
        mean = r.download_mean(0)
        assert np.array_equal(img[j == 0], mean[j == 0])  # the mean identity holds tile by tile
        r.reset()
        ar.run_schedule(r, classes)
        s = r.resolve_robust()
        _assert_tiles_are_uniform_jobs(r, ar.class_frames(classes), ref)
        assert s.n_frames == 35 and s.n_pixels == 96 * 64


def test_refusals_leave_the_context_usable():
    s = scenes.cornell_box(64, 48)

    def code(fn):
        with pytest.raises(api.ReneError) as e:
            fn()
        assert str(e.value).split(": ", 1)[1].strip()  # a message
        return e.value.code

    with api.Renderer(s) as r:
        assert code(r.resolve_robust) == -1      # no frames
        assert code(r.download_robust) == -1     # no resolve yet
        assert code(r.robust_tiles) == -1
        r.render(0, 1)
        one = r.resolve_robust()                 # one frame, k = 1: the plain mean
        assert one.n_trimmed == 0 and one.kept_energy == 1.0 and np.array_equal(r.download_robust(), r.download_mean(0))
        r.render(1, 15)
        assert code(lambda: r.resolve_robust(max_trim=4)) == -1
        for gain in (0.0, -1.0, float("nan"), float("inf")):
            assert code(lambda: r.resolve_robust(gain=gain)) == -1
        p = api.robust_params_default()
        p.struct_size = 12
        out = abi.RobustSummary()
        assert api.lib().rene_resolve_robust(r._h, C.byref(p), C.byref(out)) == -1 and b"struct_size" in api.lib().rene_last_error()
        ok = r.resolve_robust()                  # the context went on working through the refusals
        assert ok.n_frames == 16 and ok.n_pixels == 64 * 48 and 0 < ok.kept_energy <= 1
        buf = np.zeros(64 * 48 * 4, np.float32)
        dl = lambda what, ch, n: api.lib().rene_download_robust(r._h, what, ch, buf.ctypes.data_as(C.c_void_p), n)
        assert dl(2, 3, buf.size) == -1 and dl(-1, 3, buf.size) == -1            # bad `what`
        assert dl(abi.ROBUST_IMAGE, 1, buf.size) == -1 and dl(abi.ROBUST_IMAGE, 5, buf.size) == -1 and dl(abi.ROBUST_TRIM, 3, buf.size) == -1  # bad channels
        assert dl(abi.ROBUST_IMAGE, 3, 64 * 48 * 3 - 1) == -1 and dl(abi.ROBUST_TRIM, 1, 64 * 48 - 1) == -1  # n too small
        assert api.lib().rene_last_error()
        small = (abi.RobustTile * 3)()
        assert api.lib().rene_download_robust_tiles(r._h, small, 3) == -1  # the grid is 2 x 2
        assert dl(abi.ROBUST_IMAGE, 4, buf.size) == 0 and r.robust_tiles().shape == (2, 2) and r.download_robust().any()
        r.reset()
        assert code(r.download_robust) == -1     # reset: no resolve, no frames
        assert code(r.robust_tiles) == -1
        assert code(r.resolve_robust) == -1
        # an exchange consumes the chains
        r.comm_init(1, 0, api.comm_unique_id())
        r.render(0, 16)
        assert r.resolve_robust().as_dict() == ok.as_dict()
        r.gather_tiles(0)
        assert code(r.resolve_robust) == -4      # RENE_ERR_UNSUPPORTED, until the reset
        r.reset()
        r.render(0, 16)
        assert r.resolve_robust().as_dict() == ok.as_dict()
    with api.Renderer(s, shard_mode=abi.SHARD_FRAMES, shard_rank=0, shard_count=2) as r:
        r.render(0, 32)
        assert code(r.resolve_robust) == -4      # a frame shard holds a share of every pixel's frames
        assert r.download(0).max() > 0


QUALITY = {"veach": (lambda: scenes.veach_mis(96, 54), 32), "fog": (lambda: scenes.cornell_fog(64, 64), 16)}


@pytest.mark.parametrize("name", list(QUALITY))
def test_robust_halves_the_error_on_the_device(name):
    """Against a 2048-frame render from frame 100000 on the device, default seed: relMSE(robust) <= 0.5 relMSE(plain).  The CPU oracle's chains gave
    ratios of 0.021 (veach-mis @ 32) and 0.15 (fog @ 16), tests/test_robust_host.py."""
    make, spp = QUALITY[name]
    with api.Renderer(make()) as r:
        r.render(100000, 2048)
        ref = r.download(0).astype(np.float64) / 2048
        r.reset()
        r.render(0, spp)
        s = r.resolve_robust()
        plain, robust = r.download_mean(0), r.download_robust()
    e_plain, e_robust = relmse(plain, ref), relmse(robust, ref)
    print(f"{name} @ {spp}: relMSE plain {e_plain:.4f}, robust {e_robust:.4f} (ratio {e_robust / e_plain:.4f}); energy plain {plain.mean() / ref.mean():.3f}, "
          f"robust {robust.mean() / ref.mean():.3f}; kept_energy {s.kept_energy:.3f}; pixels trimmed {s.n_trimmed / s.n_pixels:.3f}")
    assert e_robust <= 0.5 * e_plain, (e_robust, e_plain)


def test_cli_robust_and_trim_map(hip_lib, tmp_path):
    from PIL import Image
    scene = os.path.join(GOLDEN, "sample_scenes", "cornell-box", "scene.pbrt")
    size = ["--width", "80", "--height", "80"]  # the Film is square: the projection is not rescaled
    png = lambda name: np.asarray(Image.open(tmp_path / name))
    p = subprocess.run([CLI, scene, *size, "--spp", "16", "--robust", "--trim-map", str(tmp_path / "t.png"), "--out", str(tmp_path / "r.png")],
                       capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    ls = loader.load_pbrt(scene)
    ls.desc.xresolution = ls.desc.yresolution = ls.xres = ls.yres = 80
    with api.Renderer(ls) as r:
        r.render(0, 16)
        s = r.resolve_robust()
        mean, j = r.download_robust(), r.download_robust(abi.ROBUST_TRIM)
        plain = api.to_rgb8(r.download(0), 16)
    assert np.array_equal(png("r.png"), api.to_rgb8(mean * np.float32(16), 16))
    assert not np.array_equal(png("r.png"), plain)
    grey = png("t.png")
    assert grey.shape == (80, 80) and grey.dtype == np.uint8 and np.array_equal(grey, (85 * j).astype(np.uint8)) and grey.max() == 255
    m = re.search(r"^INFO robust resolve: kept energy (\S+), (\S+) % of the pixels trimmed", p.stderr, re.M)
    assert m, p.stderr
    assert float(m.group(1)) == pytest.approx(s.kept_energy, abs=1e-4) and float(m.group(2)) == pytest.approx(100 * s.n_trimmed / s.n_pixels, abs=1e-2)
    # the parameters; with --target-noise and --adaptive the robust image is written as well
    p = subprocess.run([CLI, scene, *size, "--spp", "16", "--robust", "--robust-max-trim", "0", "--out", str(tmp_path / "m0.png")], capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0 and "kept energy 1.0000, 0.00 %" in p.stderr, p.stderr
    assert np.array_equal(png("m0.png"), plain)
    p = subprocess.run([CLI, scene, *size, "--spp", "48", "--batch", "16", "--target-noise", "0.05", "--adaptive", "--robust", "--robust-gain", "0.5",
                        "--out", str(tmp_path / "a.png")], capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0 and "INFO robust resolve: kept energy" in p.stderr and png("a.png").shape == (80, 80, 3), p.stderr
    # two tile shards: resolved before the exchange, placed on the host -- the same image
    p = subprocess.run([CLI, scene, *size, "--spp", "16", "--robust", "--gpus", "2", "--trim-map", str(tmp_path / "t2.png"), "--out", str(tmp_path / "r2.png")],
                       capture_output=True, text=True, cwd=tmp_path)
    if p.returncode == 0:  # one GPU on the test box: the CLI refuses more devices than it sees
        assert np.array_equal(png("r2.png"), png("r.png")) and np.array_equal(png("t2.png"), grey)
        assert f"kept energy {float(m.group(1)):.4f}" in p.stderr
    else:
        assert "GPU" in p.stderr or "device" in p.stderr
    # the filter reads the chains, not this image
    p = subprocess.run([CLI, scene, *size, "--spp", "16", "--robust", "--denoiser", "atrous"], capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 2 and "--robust" in p.stderr
