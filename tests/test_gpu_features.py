"""GPU: the denoiser hand-off (rene_export_features) against its specification -- the numpy restatement of tests/features_reference.py in
np.float32, fed with the device's own frame chains rebuilt through the public ABI, BIT FOR BIT in both layouts and both element formats -- and its
contract: the three default features are rene_download_mean; uneven tiles are shorter uniform jobs; the tile shards of one device fill one
caller-owned tensor; read-only and independent of how a job is cut into calls; a bad destination never reaches a kernel; the variance channel
agrees with the noise estimate; and the command line's PFM files."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_reference as ar
import features_reference as fr
from conftest import GOLDEN, ROOT
from rene_amd import abi, api, loader, scenes

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
ALL = abi.FEATURE_ALL
LAYOUTS = ("hwc", "chw")


def job(r, spp, first=0):
    """Renders frames first .. first + spp - 1 on r and returns what the restatement takes: the job's chains rebuilt on the device -- for chain c,
    reset, render every frame f = c (mod 8) on its own, download: the other chains hold 0 and adding 0 is exact, so the download IS C_c bit for
    bit (the trick of tests/test_gpu_noise.py) -- their counts, and the job's resolved normal and albedo sums.  r is left holding the job."""
    chains = np.zeros((8, r.yres, r.xres, 3), np.float32)
    for c in range(8):
        r.reset()
        for f in range(first, first + spp):
            if f % 8 == c:
                r.render(f, 1)
        chains[c] = r.download(0)
    r.reset()
    r.render(first, spp)
    acc = chains[0].copy()
    for c in range(1, 8):
        acc += chains[c]
    assert np.array_equal(acc, r.download(0))  # the rebuilt chains are the job's chains
    return chains, fr.chain_counts(spp, first), r.download(1), r.download(2)


def hwc(t, layout):
    return t if layout == "hwc" else np.moveaxis(t, 0, -1)


@pytest.mark.parametrize("spp", (12, 5, 1))
def test_ragged_tiles_every_feature_layout_and_format(spp):
    """cornell_box(100, 70): a 4 x 3 tile grid, ragged on the right and at the bottom; 12 frames (chains of 2 and 1), 5 (k = 5, halves of 3 and 2), 1."""
    with api.Renderer(scenes.cornell_box(100, 70)) as r:
        want = fr.features(*job(r, spp), dtype=np.float32)
        means = {fr.COLOR: r.download_mean(0), fr.ALBEDO: r.download_mean(2), fr.NORMAL: r.download_mean(1)}
        sl = fr.channel_slices(ALL)
        for layout in LAYOUTS:
            got = r.features(ALL, "f32", layout)
            ref = fr.tensor(want, ALL, layout)
            assert got.dtype == np.float32 and got.shape == ref.shape == ((70, 100, 17) if layout == "hwc" else (17, 70, 100))
            diff = hwc(got != ref, layout).reshape(-1, 17).any(axis=0)
            print(f"cornell @ {spp} {layout}: channels that differ from the restatement {np.flatnonzero(diff).tolist()}")
            assert np.array_equal(got, ref), (layout, spp)  # bit for bit: no tolerance
            for bit, mean in means.items():
                assert np.array_equal(hwc(got, layout)[..., sl[bit]], mean), (layout, fr.NAMES[bit])
            half = r.features(ALL, "f16", layout)
            assert half.dtype == np.float16 and half.shape == got.shape
            assert np.array_equal(half, np.clip(got, -65504, 65504).astype(np.float16)), layout
            # a mask picks its channels and packs them in bit order
            for mask in (abi.FEATURE_DEFAULT, fr.ALBEDO | fr.VARIANCE | fr.HALF_B | fr.FRAMES, fr.VARIANCE):
                pick = np.concatenate([np.arange(17)[s] for b, s in sl.items() if mask & b])
                assert np.array_equal(hwc(r.features(mask, "f32", layout), layout), hwc(got, layout)[..., pick]), (layout, mask)
                assert np.array_equal(hwc(r.features(mask, "f16", layout), layout), hwc(half, layout)[..., pick]), (layout, mask)
        assert np.array_equal(r.features(), hwc(got, "chw")[..., :9])  # the defaults: COLOR | ALBEDO | NORMAL, fp32, [H][W][C]
        g = hwc(got, "chw")
        assert (g[..., sl[fr.FRAMES]] == spp).all() and g[..., sl[fr.COLOR]].max() > 0 and g[..., sl[fr.ALBEDO]].max() > 0 and np.abs(g[..., sl[fr.NORMAL]]).max() > 0
        v = g[..., sl[fr.VARIANCE]]
        if spp == 1:
            assert not v.any() and not g[..., sl[fr.HALF_B]].any() and np.array_equal(g[..., sl[fr.HALF_A]], g[..., sl[fr.COLOR]])
        else:
            assert (v >= 0).all() and v.max() > 0
            hv = hwc(half, "chw")[..., sl[fr.VARIANCE]]
            assert ((hv > 0) & (hv < np.float16(6.1e-5))).any()  # the dark pixels' variance: fp16 subnormals, kept


FAMILIES = {
    "fog": (lambda: scenes.cornell_fog(64, 64), 0),                                 # volpath
    "dragon": (lambda: scenes.dragon_class(96, 64, 20, 22), 0),                     # BVH traversal-restart kernel
    "dragon-wavefront": (lambda: scenes.dragon_class(96, 64, 20, 22), abi.FLAG_WAVEFRONT),  # the stage-separated integrator
}


@pytest.mark.parametrize("name", list(FAMILIES))
def test_kernel_families(name):
    make, flags = FAMILIES[name]
    mask = abi.FEATURE_DEFAULT | abi.FEATURE_VARIANCE
    with api.Renderer(make(), flags=flags) as r:
        want = fr.features(*job(r, 12), dtype=np.float32)
        for layout in LAYOUTS:
            got = r.features(mask, "f32", layout)
            assert np.array_equal(got, fr.tensor(want, mask, layout)), (name, layout)
        assert want[fr.VARIANCE].max() > 0 and want[fr.ALBEDO].max() > 0


def test_no_aov_guides_are_zero():
    with api.Renderer(scenes.cornell_box(64, 48), flags=abi.FLAG_NO_AOV) as r:
        r.render(0, 12)
        got = r.features(ALL, "f32", "chw")
        assert not got[3:9].any() and np.array_equal(np.moveaxis(got[0:3], 0, -1), r.download_mean(0)) and got[9].max() > 0


def test_uneven_tiles_are_shorter_uniform_jobs():
    """The 96 x 64 class layout of tests/test_gpu_adaptive.py (a 3 x 2 grid): class A switched off before the first frame (N_t = 0), class B after 16
    frames, the rest render 24."""
    make = lambda: scenes.cornell_box(96, 64)
    classes = ar.tile_classes(96, 64)
    ref = {}
    with api.Renderer(make()) as u:
        for n in (16, 24):
            u.reset()
            u.render(0, n)
            ref[n] = (u.features(ALL, "f32", "hwc"), u.features(ALL, "f16", "chw"))
    with api.Renderer(make()) as r:
        r.set_active_tiles(classes != "A")
        r.render(0, 16)
        r.set_active_tiles((classes != "A") & (classes != "B"))
        r.render(16, 8)
        frames = np.where(classes == "A", 0, np.where(classes == "B", 16, 24))
        assert np.array_equal(r.tile_frames(), frames) and set(frames.ravel().tolist()) == {0, 16, 24}
        got, half = r.features(ALL, "f32", "hwc"), r.features(ALL, "f16", "chw")
        mean = r.download_mean(0)
        for t, sl in ar.tile_slices(96, 64):
            n = int(frames[t])
            if n == 0:
                assert not got[sl].any() and not half[(slice(None),) + sl].any(), t  # FRAMES included
                continue
            assert np.array_equal(got[sl], ref[n][0][sl]), (t, n)
            assert np.array_equal(half[(slice(None),) + sl], ref[n][1][(slice(None),) + sl]), (t, n)
        per_pixel = np.kron(frames, np.ones((32, 32)))[:64, :96].astype(np.float32)
        assert np.array_equal(got[..., 16], per_pixel) and np.array_equal(half[16], per_pixel.astype(np.float16))
        assert np.array_equal(got[..., 0:3], mean)  # every pixel over its own tile's N_t


def test_tile_shards_fill_one_tensor():
    import torch
    s = scenes.cornell_box(100, 70)  # 4 x 3 tiles, ragged on both sides
    with api.Renderer(s) as whole, api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=0, shard_count=2) as s0, \
            api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=1, shard_count=2) as s1:
        for r in (whole, s0, s1):
            r.render(0, 12)
        owner_px = np.zeros((70, 100), int)
        for t, sl in ar.tile_slices(100, 70):
            owner_px[sl] = (t[0] * 4 + t[1]) % 2
        for dtype, tdtype, layout in (("f32", torch.float32, "hwc"), ("f16", torch.float16, "chw")):
            want = whole.features(ALL, dtype, layout)
            t = torch.full(want.shape, -7.0, dtype=tdtype, device="cuda:0")  # a value no feature takes: every element must be written
            assert s0.features_into(t, ALL, layout) is t
            part = t.cpu().numpy()
            mine = owner_px == 0
            assert np.array_equal(hwc(part, layout)[mine], hwc(want, layout)[mine]) and (hwc(part, layout)[~mine] == -7).all()  # the other shard's tiles: untouched
            s1.features_into(t, ALL, layout)
            assert np.array_equal(t.cpu().numpy(), want), (dtype, layout)
            for rank, r in enumerate((s0, s1)):  # the library's own buffer: zero outside the shard's tiles
                own = hwc(r.features(ALL, dtype, layout), layout)
                mine = owner_px == rank
                assert np.array_equal(own[mine], hwc(want, layout)[mine]) and not own[~mine].any(), (rank, dtype, layout)
            w = torch.empty(want.shape, dtype=tdtype, device="cuda:0")
            whole.features_into(w, ALL, layout)
            assert np.array_equal(w.cpu().numpy(), want)
        # the Python side's own checks
        with pytest.raises(ValueError):
            whole.features_into(torch.empty((70, 100, 9), device="cuda:0"), ALL)            # shape
        with pytest.raises(ValueError):
            whole.features_into(torch.empty((70, 100, 17)), ALL)                            # a host tensor
        with pytest.raises(ValueError):
            whole.features_into(torch.empty((17, 70, 100), device="cuda:0").permute(1, 2, 0), ALL)  # not contiguous
        with pytest.raises(TypeError):
            whole.features_into(torch.empty((70, 100, 17), dtype=torch.float64, device="cuda:0"), ALL)


def test_independent_of_the_cut_and_read_only():
    s = scenes.cornell_box(100, 70)
    stat = lambda r: {k: v for k, v in r.stats().as_dict().items() if k != "sclk_mhz"}
    with api.Renderer(s) as r, api.Renderer(s) as cut:
        r.render(0, 12)
        cut.render(0, 5)
        cut.render(5, 7)
        before, st = [r.download(l) for l in range(3)], stat(r)
        a = r.features(ALL, "f32", "chw")
        for l in range(3):
            assert np.array_equal(r.download(l), before[l])
        assert stat(r) == st and st["frames"] == 12
        assert np.array_equal(r.features(ALL, "f32", "chw"), a)  # deterministic
        assert np.array_equal(cut.features(ALL, "f32", "chw"), a)
        ptr, n = r.features_buffer()
        assert ptr and n == 17 * 70 * 100 * 4
        r.features(abi.FEATURE_VARIANCE, "f16")
        assert r.features_buffer()[1] == 70 * 100 * 2
        r.render(12, 4)  # later frames are what they are without the call
        cut.render(12, 4)
        for l in range(3):
            assert np.array_equal(r.download(l), cut.download(l))


def test_refusals_launch_nothing_and_leave_the_context_usable():
    import torch
    s = scenes.cornell_box(64, 48)
    L = api.lib()
    need = 64 * 48 * 9 * 4

    def code(fn):
        with pytest.raises(api.ReneError) as e:
            fn()
        assert str(e.value).split(": ", 1)[1].strip()  # a message
        return e.value.code

    with api.Renderer(s) as r:
        assert code(r.features_buffer) == -1            # no export yet
        zero = r.features(ALL)                          # no frames: every tile has N_t = 0, all zeros
        assert not zero.any() and r.features_buffer()[1] == zero.nbytes
        r.render(0, 12)
        want = r.features()
        p = api.feature_params_default()
        export = lambda p, ptr, n: L.rene_export_features(r._h, C.byref(p), C.c_void_p(ptr), n)
        host = np.full(64 * 48 * 9, -7.0, np.float32)
        assert export(p, host.ctypes.data, host.nbytes) == -1 and L.rene_last_error()  # a host pointer never reaches a kernel
        assert (host == -7).all()
        t = torch.full((48, 64, 9), -7.0, device="cuda:0")
        assert export(p, t.data_ptr(), need - 1) == -1 and b"dst_bytes" in L.rene_last_error()  # one byte short
        assert export(p, t.data_ptr() + 2, need) == -1                                           # not aligned to the element
        pinned = torch.full((48, 64, 9), -7.0).pin_memory()
        assert export(p, pinned.data_ptr(), need) == -1 and (pinned == -7).all()                 # host memory the runtime knows
        for field, bad in (("struct_size", 12), ("features", 0), ("features", 128), ("features", 1 << 31 | 1), ("format", 2), ("layout", 2)):
            q = api.feature_params_default()
            setattr(q, field, bad)
            assert export(q, t.data_ptr(), need) == -1 and L.rene_last_error(), (field, bad)
        assert (t == -7).all().item()                   # nothing was launched on it
        assert export(p, t.data_ptr(), need) == 0 and np.array_equal(t.cpu().numpy(), want)
        small = np.zeros(8, np.float32)
        assert L.rene_download_features(r._h, small.ctypes.data_as(C.c_void_p), small.nbytes) == -1
        assert np.array_equal(r.features(), want)       # the context went on working through the refusals
        r.reset()
        assert code(r.features_buffer) == -1            # reset: no export
        out = np.zeros(want.size, np.float32)
        assert L.rene_download_features(r._h, out.ctypes.data_as(C.c_void_p), out.nbytes) == -1
        # an exchange consumes the chains
        r.comm_init(1, 0, api.comm_unique_id())
        r.render(0, 12)
        assert np.array_equal(r.features(), want)
        r.gather_tiles(0)
        assert code(r.features) == -4                   # RENE_ERR_UNSUPPORTED, until the reset
        r.reset()
        r.render(0, 12)
        assert np.array_equal(r.features(), want)
    with api.Renderer(s, shard_mode=abi.SHARD_FRAMES, shard_rank=0, shard_count=2) as r:
        r.render(0, 16)
        assert code(r.features) == -4                   # a frame shard holds a share of every pixel's frames
        assert code(r.features_buffer) == -1
        assert r.download(0).max() > 0


@pytest.mark.parametrize("name", list(fr.SPREAD_CASES))
def test_variance_agrees_with_the_noise_estimate(name):
    """Per tile, the VARIANCE channel summed on the host in fp64 against rene_estimate_noise's sum_var.  Both are fp32 evaluations of one formula (the
    estimate multiplies by reciprocals and adds a tile's pixels in fp32, the export divides and is added here in fp64), so the bound is twice a
    one-sided bound, and that is 16 x the restatement's own fp32-vs-fp64 spread of these tile sums on the CPU oracle's chains of these four cases:
    4.5e-8 (features_reference.VARIANCE_SPREAD; tests/test_features_host.py measures it: 3.0e-8 / 7.2e-9, 2.1e-8 / 3.7e-8, 1.7e-8 / 1.4e-8, 3.6e-8 / 4.5e-8 for the fp32 pixels summed
    in fp64 / in fp32), as max over tiles of |difference| / (|value| + the largest tile's value).  Bound: 2 * 16 * 4.5e-8 = 1.44e-6.  (Not tuned on the
    device's output.)"""
    scene, args, spp = fr.SPREAD_CASES[name]
    bound = 2 * 16 * fr.VARIANCE_SPREAD
    with api.Renderer(getattr(scenes, scene)(*args)) as r:
        r.render(0, spp)
        r.estimate_noise()
        a = r.noise_tiles()["sum_var"].astype(np.float64)
        v = r.features(abi.FEATURE_VARIANCE, "f32", "chw")[0]
    mine = fr.tile_sums(v)
    err = np.abs(mine - a) / (np.abs(a) + a.max())
    print(f"{name} @ {spp}: VARIANCE tile sums against sum_var, max {err.max():.3g} of |value| + largest tile (bound {bound:.3g})")
    assert a.max() > 0 and np.isfinite(mine).all()
    assert err.max() <= bound, (name, float(err.max()))


def read_pfm(path):
    """A PFM as [H][W][C] (or [H][W]) float32, rows top first."""
    raw = open(path, "rb").read()
    kind, size, scale, data = raw.split(b"\n", 3)
    w, h = map(int, size.split())
    assert kind in (b"PF", b"Pf") and float(scale) == -1.0  # little-endian, scale 1
    ch = 3 if kind == b"PF" else 1
    a = np.frombuffer(data, "<f4")
    assert a.size == w * h * ch
    a = a.reshape(h, w, ch)[::-1]  # the file's rows are bottom first
    return a if ch == 3 else a[..., 0]


def test_cli_features(hip_lib, tmp_path):
    from PIL import Image
    scene = os.path.join(GOLDEN, "sample_scenes", "cornell-box", "scene.pbrt")
    size = ["--width", "80", "--height", "80"]  # the Film is square: the projection is not rescaled
    p = subprocess.run([CLI, scene, *size, "--spp", "16", "--features", str(tmp_path / "p"), "--out", str(tmp_path / "r.png")], capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    ls = loader.load_pbrt(scene)
    ls.desc.xresolution = ls.desc.yresolution = ls.xres = ls.yres = 80
    with api.Renderer(ls) as r:
        r.render(0, 16)
        want = r.features(ALL, "f32", "hwc")
    sl = fr.channel_slices(ALL)
    for bit, name in fr.NAMES.items():
        got = read_pfm(tmp_path / f"p.{name}.pfm")
        ref = want[..., sl[bit]]
        assert got.shape == ((80, 80, 3) if fr.WIDTH[bit] == 3 else (80, 80)), name
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(ref if fr.WIDTH[bit] == 3 else ref[..., 0]).view(np.uint32)), name  # bit for bit
    assert want[..., sl[fr.COLOR]].max() > 0 and want[..., sl[fr.VARIANCE]].max() > 0
    # an adaptive job: every pixel over its own tile's frames, and .frames.pfm is the sample map per pixel
    p = subprocess.run([CLI, scene, *size, "--spp", "48", "--batch", "16", "--target-noise", "0.05", "--adaptive", "--features", str(tmp_path / "a"),
                        "--sample-map", str(tmp_path / "s.png"), "--out", str(tmp_path / "a.png")], capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    frames = read_pfm(tmp_path / "a.frames.pfm")
    tiles = np.zeros((3, 3), np.int64)
    for t, s in ar.tile_slices(80, 80):
        assert (frames[s] == frames[s][0, 0]).all(), t  # one count per tile
        tiles[t] = int(frames[s][0, 0])
    assert tiles.min() >= 16 and tiles.max() <= 48 and not (tiles % 8).any()
    grey = np.asarray(Image.open(tmp_path / "s.png"))
    assert np.array_equal(grey, np.floor(255.0 * tiles / tiles.max() + 0.5).astype(np.uint8))
    assert read_pfm(tmp_path / "a.color.pfm").max() > 0
    # with --robust the features still describe the plain mean
    p = subprocess.run([CLI, scene, *size, "--spp", "16", "--robust", "--features", str(tmp_path / "q"), "--out", str(tmp_path / "q.png")], capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0 and np.array_equal(read_pfm(tmp_path / "q.color.pfm"), read_pfm(tmp_path / "p.color.pfm")), p.stderr
