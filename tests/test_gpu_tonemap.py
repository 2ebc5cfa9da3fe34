"""GPU: the tone-mapped output transform and the luminance histogram on the device (rene_output_tonemapped, rene_luminance_histogram,
include/rene_hip.h) against the host functions of the same arithmetic (rene_tonemap_rgb8, rene_luminance_histogram_host), which
tests/test_tonemap_host.py holds against the numpy restatement.  Everything is array_equal on bytes and integers: the probe of the per-pixel device
function, rendered images, crafted chains (the edge film; means on and beside every bin edge of the histogram), adaptive tile counts with a zero
tile, tile shards into one tensor and their histograms' sum, the denoised and robust sources, the refusals, and the command line against its own
host path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_reference as ar
import chain_reference as cr
import tonemap_reference as tr
from conftest import GOLDEN, ROOT
from rene_amd import abi, api, scenes

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
H, W = 130, 161      # tests/chain_reference.py's film: 5 x 6 = 30 tiles, the last column one pixel wide
FIRST = 3
OPS = list(tr.OPS)
EXPOSURES = (0.375, -3.0)  # EV: 3 and -24 eighth-stops, the factors 2^(3/8) and 2^-3
E8 = (3, -24)


def code(fn):
    with pytest.raises(api.ReneError) as e:
        fn()
    assert str(e.value).split(": ", 1)[1].strip()  # a message
    return e.value.code


def same(got, want, label):
    assert got.shape == want.shape and got.dtype == np.uint8, label
    bad = np.argwhere(got != want)
    assert bad.size == 0, (label, len(bad), bad[:4].tolist())


def check_tonemapped(r, source, means, label, ops=OPS):
    """rgb8(source, tonemap=, exposure=) for every operator x format x two exposures against rene_tonemap_rgb8 of `means` [H][W][3]."""
    for op in ops:
        for ev, e8 in zip(EXPOSURES, E8):
            want = api.tonemap_rgb8(means, op, api.exposure_scale(e8))
            same(r.rgb8(source, tonemap=op, exposure=ev), want, (label, op, ev))
            rgba = r.rgb8(source, alpha=True, tonemap=op, exposure=ev)
            assert rgba.shape == want.shape[:2] + (4,) and (rgba[..., 3] == 255).all(), (label, op, ev)
            same(np.ascontiguousarray(rgba[..., :3]), want, (label, op, ev, "rgba"))
    same(r.rgb8(source, tonemap="reinhard", white=1.5), api.tonemap_rgb8(means, "reinhard", 1.0, 1.5), (label, "white"))


def check_histogram(r, source, means, label):
    """luminance_stats(source) against the host histogram of `means`; returns the stats."""
    got, want = r.luminance_stats(source), api.luminance_histogram_host(means)
    assert np.array_equal(api.luminance_counts(got), api.luminance_counts(want)) and got.n_dark == want.n_dark, label
    assert got.n_pixels == want.n_pixels == got.n_dark + int(api.luminance_counts(got).sum()) and got.struct_size == C.sizeof(got), label
    return got


# ---- the probe: the device function, pixel by pixel ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe_pixels():
    return tr.value_set(api.output_thresholds())


@pytest.mark.parametrize("op", OPS)
def test_probe_equals_the_host_function(probe_pixels, op):
    v = probe_pixels
    for scale in tr.SCALES:
        for white in ((4.0, 1.5) if op == "reinhard" else (4.0,)):
            got, want = api.tonemap_probe(v, op, scale, white), api.tonemap_rgb8(v, op, scale, white)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (op, float(scale), white, len(bad), [(v[i].tolist(), int(got[i, c]), int(want[i, c])) for i, c in bad[:4]])
            assert len(np.unique(want)) == 256


# ---- rendered images ---------------------------------------------------------------------------------------------------------------------------------
RENDERED = {
    "cornell": (lambda: scenes.cornell_box(100, 70), 12),    # 4 x 3 ragged tiles; the small-scene item loop
    "dragon": (lambda: scenes.dragon_class(240, 136), 16),   # the traversal-restart kernel
}


@pytest.mark.parametrize("name", list(RENDERED))
def test_rendered_images(name):
    make, spp = RENDERED[name]
    with api.Renderer(make()) as r:
        r.render(0, spp)
        before = [r.download(l) for l in range(3)]
        means = r.download_mean(0)
        plain = r.rgb8()
        check_tonemapped(r, "radiance", means, name)
        same(r.rgb8(tonemap="clamp"), plain, (name, "clamp at scale 1 is rgb8()"))
        same(r.rgb8(exposure=0.0), plain, name)
        same(r.rgb8(alpha=True, tonemap="clamp"), r.rgb8(alpha=True), name)
        assert (r.rgb8(tonemap="aces", exposure=1.0) != plain).any() and len(np.unique(r.rgb8(tonemap="reinhard"))) > 8
        st = check_histogram(r, "radiance", means, name)
        assert st.n_pixels == means.shape[0] * means.shape[1] and int(api.luminance_counts(st).sum()) > st.n_pixels // 2
        e8 = api.auto_exposure_e8(st)
        assert e8 == tr.auto_exposure_e8(api.luminance_counts(st))
        same(r.rgb8(tonemap="aces", exposure="auto"), api.tonemap_rgb8(means, "aces", api.exposure_scale(e8)), (name, "auto"))
        same(r.rgb8(tonemap="aces", exposure="auto", key=-12), api.tonemap_rgb8(means, "aces", api.exposure_scale(e8 + 8)), (name, "auto, key"))
        for l in range(3):
            assert np.array_equal(r.download(l), before[l])  # the accumulation state is read, never written
        r.render(spp, 4)  # ... and the context renders on
        same(r.rgb8(tonemap="reinhard"), api.tonemap_rgb8(r.download_mean(0), "reinhard"), (name, "rendered on"))


# ---- crafted chains ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_film():
    edge, _, _ = cr.edge_chains(H, W, seed=0)
    return edge


def test_edge_film(edge_film):
    chains = cr.for_counts(edge_film, cr.chain_counts(12, FIRST))
    with api.Renderer(scenes.cornell_box(W, H)) as r:
        r.load_chains(chains, FIRST, 12)
        means = r.download_mean(0)
        flat = means.reshape(-1)
        assert np.isnan(flat).any() and np.isposinf(flat).any() and np.isneginf(flat).any() and (flat < 0).any()
        assert ((np.abs(flat) > 0) & (np.abs(flat) < 1.1754942e-38)).any(), "the edge film holds denormal means"
        check_tonemapped(r, "radiance", means, "edge")
        same(r.rgb8(tonemap="clamp"), r.rgb8(), "edge, clamp")
        st = check_histogram(r, "radiance", means, "edge")
        assert st.n_dark > 0 and st.n_pixels == H * W


def test_means_on_and_beside_every_bin_edge():
    px = tr.edge_pixels()  # [n][3]: luminances on, one ulp below and one ulp above every edge 2^k (1 + j / 8)
    dark = np.array([[0, 0, 0], [-0.0, -0.0, -0.0], [-1, 0.1, 0], [np.nan, 1, 1], [-np.inf, 0, 0], [np.inf, 0, -np.inf], [1e-45, 0, 0]], np.float32)
    values = np.concatenate([px, dark]).reshape(-1)
    film = cr.value_films(values, H, W)
    assert len(film) == 1
    with api.Renderer(scenes.cornell_box(W, H)) as r:
        r.load_chains(cr.single_chain_load(film[0], 1.0), 0, 1)
        means = r.download_mean(0)
        assert np.array_equal(means.reshape(-1)[:values.size].view(np.uint32), values.view(np.uint32))  # one frame: the means are the film, bit for bit
        with np.errstate(all="ignore"):
            lum = tr.lum3(means[..., 0], means[..., 1], means[..., 2])
        edges = tr.bin_edges()
        for t in (edges, np.nextafter(edges, np.float32(0)), np.nextafter(edges, np.float32(np.inf))):
            assert np.isin(t, lum).all()
        st = check_histogram(r, "radiance", means, "bin edges")
        counts, n_dark = tr.histogram(means)  # ... and the restatement itself
        assert np.array_equal(api.luminance_counts(st), counts) and st.n_dark == n_dark and (counts > 0).all()
        assert st.n_dark >= H * W - len(px) - len(dark)  # the film's padding is zero: dark
        check_tonemapped(r, "radiance", means, "bin edges", ops=["reinhard"])


def test_adaptive_tile_counts(edge_film):
    tf = ar.class_frames(ar.tile_classes(W, H))
    assert sorted(np.unique(tf)) == [0, 11, 19, 35]
    chains = cr.for_tile_frames(edge_film, FIRST, tf)
    with api.Renderer(scenes.cornell_box(W, H)) as r:
        r.load_chains(chains, FIRST, 35, tf)
        means = r.download_mean(0)
        check_tonemapped(r, "radiance", means, "adaptive")
        st = check_histogram(r, "radiance", means, "adaptive")
        got = r.rgb8(tonemap="aces", exposure=2.0)
        zero_px = 0
        for (ty, tx), (rows, cols) in ar.tile_slices(W, H):
            if tf[ty, tx] == 0:  # N_t == 0: black, and counted dark
                assert not got[rows, cols].any(), (ty, tx)
                zero_px += (rows.stop - rows.start) * (cols.stop - cols.start)
        assert st.n_dark >= zero_px > 0


# ---- tile shards --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [2, 3])
def test_tile_shards_fill_one_tensor_and_their_histograms_add_up(shards):
    import torch
    s = scenes.cornell_box(100, 70)
    with api.Renderer(s) as whole:
        whole.render(0, 12)
        st_whole = whole.luminance_stats()
        e8 = api.auto_exposure_e8(st_whole)
        want = {(op, alpha): whole.rgb8(alpha=alpha, tonemap=op, exposure=e8 / 8) for op in OPS for alpha in (False, True)}
        same(want["aces", False], whole.rgb8(tonemap="aces", exposure="auto"), "auto")
    tiles = np.arange(12).reshape(3, 4)
    rs = [api.Renderer(s, shard_mode=abi.SHARD_TILES, shard_rank=k, shard_count=shards) for k in range(shards)]
    try:
        for r in rs:
            r.render(0, 12)
        parts = [r.luminance_stats() for r in rs]
        total = api.luminance_combine(parts)
        assert np.array_equal(api.luminance_counts(total), api.luminance_counts(st_whole)) and total.n_dark == st_whole.n_dark
        assert total.n_pixels == st_whole.n_pixels == 7000 and all(0 < p.n_pixels < 7000 for p in parts)
        assert api.auto_exposure_e8(total) == e8  # the shards' combined statistics choose the unsharded exposure
        for (op, alpha), image in want.items():
            t = torch.full((70, 100, 4 if alpha else 3), 0xA5, dtype=torch.uint8, device="cuda:0")
            for k, r in enumerate(rs):
                assert r.rgb8_into(t, alpha=alpha, tonemap=op, exposure=e8 / 8) is t
                got = t.cpu().numpy()
                for (ty, tx), (rows, cols) in ar.tile_slices(100, 70):
                    if tiles[ty, tx] % shards <= k:
                        assert np.array_equal(got[rows, cols], image[rows, cols]), (op, alpha, k, ty, tx)
                    else:
                        assert (got[rows, cols] == 0xA5).all(), (op, alpha, k, ty, tx)  # not a byte of a tile that is not its own
            assert np.array_equal(t.cpu().numpy(), image), (op, alpha)
    finally:
        for r in rs:
            r.close()


# ---- the denoised and the robust image ----------------------------------------------------------------------------------------------------------------
def test_denoised_and_robust_on_an_even_context():
    with api.Renderer(scenes.cornell_box(100, 70)) as r:
        r.render(0, 12)
        for src in ("denoised", "denoised_mean", "robust"):
            assert code(lambda: r.rgb8(src, tonemap="aces")) == -1 and code(lambda: r.luminance_stats(src)) == -1, src  # before its call has run
        r.denoise()
        with np.errstate(all="ignore"):
            dn = r.download_denoised(abi.DENOISED_RADIANCE) / np.float32(12)
        check_tonemapped(r, "denoised", dn, "denoised")
        check_histogram(r, "denoised", dn, "denoised")
        dm = r.download_denoised(abi.DENOISED_MEAN)
        check_tonemapped(r, "denoised_mean", dm, "denoised_mean", ops=["aces"])
        check_histogram(r, "denoised_mean", dm, "denoised_mean")
        assert code(lambda: r.rgb8("robust", tonemap="aces")) == -1
        r.resolve_robust()
        rb = r.download_robust()
        check_tonemapped(r, "robust", rb, "robust", ops=["reinhard"])
        check_histogram(r, "robust", rb, "robust")
        r.reset()
        for src in ("denoised", "denoised_mean", "robust"):
            assert code(lambda: r.rgb8(src, exposure=1)) == -1, src


def test_denoised_mean_under_the_class_schedule():
    classes = ar.tile_classes(100, 70)
    with api.Renderer(scenes.cornell_box(100, 70)) as r:
        ar.run_schedule(r, classes)
        assert sorted(np.unique(r.tile_frames())) == [0, 11, 19, 35]
        assert code(lambda: r.rgb8("denoised_mean", tonemap="aces")) == -1
        r.denoise_tiles()
        dm = r.download_denoised(abi.DENOISED_MEAN)
        check_tonemapped(r, "denoised_mean", dm, "denoised_mean, tiles")
        check_histogram(r, "denoised_mean", dm, "denoised_mean, tiles")
        assert code(lambda: r.rgb8("denoised", tonemap="aces")) == -4  # one count does not divide tiles that differ in theirs
        check_tonemapped(r, "radiance", r.download_mean(0), "adaptive radiance", ops=["aces"])


# ---- refusals launch nothing ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_destination_untouched():
    import torch
    L = api.lib()
    need = 100 * 70 * 3
    with api.Renderer(scenes.cornell_box(100, 70)) as r:
        r.render(0, 12)
        want = r.rgb8(tonemap="aces", exposure=1)
        t = torch.full((70, 100, 3), 0xA5, dtype=torch.uint8, device="cuda:0")
        call = lambda p, ptr=None, n=need: L.rene_output_tonemapped(r._h, C.byref(p), C.c_void_p(t.data_ptr() if ptr is None else ptr), n)

        def params(**kw):
            p = api.tonemap_params_default()
            for k, v in kw.items():
                setattr(p, k, v)
            return p

        for kw, word in (({"source": abi.OUTPUT_NORMAL}, b"NORMAL"), ({"source": abi.OUTPUT_ALBEDO}, b"ALBEDO"), ({"source": 6}, b"source"), ({"op": 3}, b"op"),
                         ({"format": 2}, b"format"), ({"struct_size": 16}, b"struct_size"), ({"white": 0.0}, b"white"), ({"white": float("nan")}, b"white")):
            assert call(params(**kw)) == -1 and word in L.rene_last_error(), kw
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert call(params(scale=bad)) == -1 and b"scale" in L.rene_last_error(), bad
        host = np.full(need, 0xA5, np.uint8)
        assert call(params(), host.ctypes.data, need) == -1 and (host == 0xA5).all()  # a host pointer never reaches a kernel
        assert call(params(), None, need - 1) == -1 and b"dst_bytes" in L.rene_last_error()  # one byte short
        assert call(params(), t.data_ptr() + 1, need) == -1 and b"aligned" in L.rene_last_error()
        st = abi.LuminanceStats()
        for src in (abi.OUTPUT_NORMAL, abi.OUTPUT_ALBEDO, 6):
            assert L.rene_luminance_histogram(r._h, src, C.byref(st)) == -1
        for src in ("normal", "albedo"):
            assert code(lambda: r.rgb8(src, tonemap="aces")) == -1 and code(lambda: r.luminance_stats(src)) == -1
        with pytest.raises(ValueError):
            r.rgb8(tonemap="filmic")
        with pytest.raises(ValueError):
            r.rgb8(exposure="bright")
        assert (t == 0xA5).all().item()  # nothing was launched on it
        same(r.rgb8_into(t, tonemap="aces", exposure=1).cpu().numpy(), want, "usable afterwards")
    with api.Renderer(scenes.cornell_box(100, 70), shard_mode=abi.SHARD_FRAMES, shard_rank=0, shard_count=2) as r:
        r.render(0, 16)
        t = torch.full((70, 100, 3), 0xA5, dtype=torch.uint8, device="cuda:0")
        assert code(lambda: r.rgb8_into(t, tonemap="aces")) == -4 and code(r.luminance_stats) == -4  # a frame shard holds a share of every pixel's frames
        assert (t == 0xA5).all().item()


# ---- the command line: the device stage against its own host path ------------------------------------------------------------------------------------
CLI_RUNS = {
    "aces-auto": ["--tonemap", "aces", "--exposure", "auto"],
    "reinhard": ["--tonemap", "reinhard", "--exposure", "1.5", "--white", "8"],
    "atrous-aces": ["--denoiser", "atrous", "--tonemap", "aces"],
}


@pytest.mark.parametrize("name", list(CLI_RUNS))
def test_cli_files_are_identical_either_way(hip_lib, tmp_path, name):
    scene = os.path.join(GOLDEN, "sample_scenes", "cornell-box", "scene.pbrt")
    files, info = {}, {}
    for mode in ("device", "host", "plain"):
        d = tmp_path / mode
        d.mkdir()
        env = {k: v for k, v in os.environ.items() if k != "RENE_HOST_OUTPUT"}
        env["RENE_DEBUG"] = "1"  # the library's log says which kernels ran
        if mode == "host":
            env["RENE_HOST_OUTPUT"] = "1"
        flags = CLI_RUNS[name] if mode != "plain" else [f for f in CLI_RUNS[name] if f in ("--denoiser", "atrous")]  # plain: the same job, no tone mapping
        p = subprocess.run([CLI, scene, "--width", "100", "--height", "70", "--spp", "16", "--out", "o.png", "--aov-albedo", "a.png", *flags], capture_output=True, text=True,
                           cwd=d, env=env)
        assert p.returncode == 0, p.stderr
        if mode == "device":  # the tone-mapped kernel made --out, the plain one the AOV; the histogram ran where the exposure is `auto`
            assert p.stderr.count("[rene] output ") == 2 and p.stderr.count(", " + CLI_RUNS[name][CLI_RUNS[name].index("--tonemap") + 1] + ", scale ") == 1, p.stderr
            assert p.stderr.count("[rene] luminance histogram ") == (1 if "auto" in flags else 0), p.stderr
        if mode == "host":
            assert "[rene] output " not in p.stderr and "[rene] luminance histogram " not in p.stderr, p.stderr
        info[mode] = [l for l in p.stderr.splitlines() if l.startswith("INFO auto exposure")]
        files[mode] = {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}
    assert set(files["device"]) == set(files["host"]) == {"o.png", "a.png"}
    for f in files["host"]:
        assert files["device"][f] == files["host"][f] and len(files["host"][f]) > 1000, (name, f)
    assert files["device"]["a.png"] == files["plain"]["a.png"]  # the AOV files are not tone-mapped
    assert files["device"]["o.png"] != files["plain"]["o.png"]
    assert info["device"] == info["host"] and len(info["device"]) == (1 if name == "aces-auto" else 0) and not info["plain"]
