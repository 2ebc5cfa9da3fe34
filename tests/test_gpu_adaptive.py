"""GPU: adaptive sampling (include/rene_hip.h: rene_set_active_tiles, rene_tile_frames, rene_download_mean, rene_estimate_noise on uneven tiles,
Renderer.render_adaptive).  The contract is exactness: a tile that was switched off after N_t frames is, bit for bit and in every layer, that
tile of a context that rendered render(0, N_t) -- on every kernel family, in tile shards, through a replayed launch and across the epoch wrap --
and its noise record is that context's record."""
import types

import numpy as np
import pytest

import adaptive_reference as ar
import noise_reference as nr
from rene_amd import abi, api, scenes

pytestmark = pytest.mark.gpu

# the five scenes of test_frame_chains_do_not_depend_on_the_cut_and_sum_to_the_frames at its sizes (one per kernel family) and three flag variants
CASES = {
    "dragon": (lambda: scenes.dragon_class(160, 90, 40, 44), 0),      # traversal-restart kernel (render_wf.inc)
    "teapot": (lambda: scenes.teapot_class(128, 72, 40, 44), 0),      # ... with the general BSDF
    "fog": (lambda: scenes.dragon_fog(128, 72, 40, 44), 0),           # volpath restart kernel
    "cornell": (lambda: scenes.cornell_box(96, 64), 0),               # Matte item-loop kernel with the frame-stream table
    "veach": (lambda: scenes.veach_mis(96, 54), 0),                   # item-loop kernel, general BSDF
    "cornell-no-aov": (lambda: scenes.cornell_box(96, 64), abi.FLAG_NO_AOV),
    "dragon-no-restart": (lambda: scenes.dragon_class(160, 90, 40, 44), abi.FLAG_NO_RESTART),  # the while-while kernel of device_code.inc
    "zoo": (lambda: scenes.material_zoo(96, 64), 0),                  # textures, environment map
    "cornell-100x70": (lambda: scenes.cornell_box(100, 70), 0),       # ragged on both sides (the noise and mean cases)
}
_uniform = {}


def uniform(name):
    """{N: (three layers, noise tile records or None)} of fresh uniform renders render(0, N) for the classes' frame counts -- computed once per case."""
    if name not in _uniform:
        make, flags = CASES[name]
        out = {}
        with api.Renderer(make(), flags=flags) as r:
            for n in sorted(set(ar.CLASS_FRAMES.values()) - {0}):
                r.reset()
                r.render(0, n)
                layers = [r.download(l) for l in range(3)]
                r.estimate_noise()
                out[n] = (layers, r.noise_tiles())
        _uniform[name] = out
    return _uniform[name]


def scheduled(name, **kw):
    make, flags = CASES[name]
    r = api.Renderer(make(), flags=flags, **kw)
    s = types.SimpleNamespace(xres=r.xres, yres=r.yres)  # the image's size, for the tile arithmetic
    classes = ar.tile_classes(s.xres, s.yres)
    ar.run_schedule(r, classes)
    return r, s, classes


def assert_tiles_equal_uniform(name, layers, classes, xres, yres, owned=None):
    ref = uniform(name)
    for t, sl in ar.tile_slices(xres, yres):
        n = ar.CLASS_FRAMES[classes[t]]
        for l in range(3):
            got = layers[l][sl]
            if n == 0 or (owned is not None and not owned[t]):
                assert not got.any(), (name, t, l)  # never rendered (or not this shard's): zeros
            else:
                assert np.array_equal(got, ref[n][0][l][sl]), (name, t, classes[t], l)


def raw(t):
    return np.ascontiguousarray(t).view(np.uint32).reshape(t.shape + (4,))


@pytest.mark.parametrize("name", ["dragon", "teapot", "fog", "cornell", "veach", "cornell-no-aov", "dragon-no-restart", "zoo"])
def test_a_masked_tile_is_exactly_a_shorter_job(name):
    r, s, classes = scheduled(name)
    with r:
        assert set(classes.ravel()) == set("ABCD")
        layers = [r.download(l) for l in range(3)]
        assert_tiles_equal_uniform(name, layers, classes, s.xres, s.yres)
        frames = ar.class_frames(classes)
        tf = r.tile_frames()
        assert tf.dtype == np.uint32 and np.array_equal(tf, frames)
        st = r.stats().as_dict()
        assert st["paths"] == int((frames.astype(np.int64) * ar.tile_pixels(s.xres, s.yres)).sum())
        assert st["frames"] == 35 and st["launches"] == 3
    # the sums of the rendered tiles are not all zero: the comparison above is not of nothing with nothing
    rendered = np.zeros((s.yres, s.xres), bool)
    for t, sl in ar.tile_slices(s.xres, s.yres):
        rendered[sl] = classes[t] != "A"
    assert layers[0][rendered].any()
    if not CASES[name][1] & abi.FLAG_NO_AOV:
        assert layers[1][rendered].any() and layers[2][rendered].any()


@pytest.mark.parametrize("name", ["cornell-100x70", "dragon"])
def test_noise_estimate_on_uneven_tiles(name):
    r, s, classes = scheduled(name)
    with r:
        est = r.estimate_noise()
        tiles = r.noise_tiles()
    ref = uniform(name)
    for t, _ in ar.tile_slices(s.xres, s.yres):
        n = ar.CLASS_FRAMES[classes[t]]
        if n == 0:
            assert not raw(tiles)[t].any(), (name, t)  # class A: not estimated
        else:
            assert np.array_equal(raw(tiles)[t], raw(ref[n][1])[t]), (name, t, classes[t])  # sum_var, sum_lum, n_pixels: the uniform context's bits
            assert tiles["n_pixels"][t] == ar.tile_pixels(s.xres, s.yres)[t]
    assert est.n_frames == 35 and est.n_chains == 8
    a, b, n = tiles["sum_var"].astype(np.float64), tiles["sum_lum"].astype(np.float64), tiles["n_pixels"].astype(np.int64)
    fig = nr.figures(a, b, n, est.luminance_floor)
    assert est.n_tiles == fig["n_tiles"] == int((classes != "A").sum()) and est.n_pixels == fig["n_pixels"]
    for k in ("sum_var", "sum_lum", "sum_weighted_q", "noise", "rel_rmse", "worst_tile_noise"):
        assert abs(getattr(est, k) - fig[k]) <= 1e-12 * abs(fig[k]), (name, k)
    assert est.worst_tile == fig["worst_tile"]


def test_download_mean():
    s = scenes.cornell_box(100, 70)
    with api.Renderer(s) as r:
        r.render(0, 12)
        for layer in range(3):
            for ch in (3, 4):
                assert np.array_equal(r.download_mean(layer, ch), r.download(layer, ch) / np.float32(12)), (layer, ch)
        assert r.download_mean(0, 3).any()
    r, s, classes = scheduled("cornell-100x70")
    with r:
        for layer in range(3):
            for ch in (3, 4):
                mean, sums = r.download_mean(layer, ch), r.download(layer, ch)
                for t, sl in ar.tile_slices(s.xres, s.yres):
                    n = ar.CLASS_FRAMES[classes[t]]
                    if n == 0:
                        assert not mean[sl].any()
                    else:
                        assert np.array_equal(mean[sl], sums[sl] / np.float32(n)), (layer, ch, t)


def test_tile_shards():
    name = "cornell-100x70"
    whole, s, classes = scheduled(name)
    with whole:
        want = [whole.download(l) for l in range(3)]
        want_frames = whole.tile_frames()
    ty, tx = classes.shape
    owner = np.arange(ty * tx).reshape(ty, tx) % 2
    shards = [scheduled(name, shard_mode=abi.SHARD_TILES, shard_rank=k, shard_count=2)[0] for k in range(2)]  # both on one card
    try:
        got_frames = []
        for k, sh in enumerate(shards):
            layers = [sh.download(l) for l in range(3)]
            assert_tiles_equal_uniform(name, layers, classes, s.xres, s.yres, owned=owner == k)
            for t, sl in ar.tile_slices(s.xres, s.yres):
                if owner[t] == k:
                    for l in range(3):
                        assert np.array_equal(layers[l][sl], want[l][sl]), (k, t, l)
            tf = sh.tile_frames()
            assert not tf[owner != k].any()
            got_frames.append(tf)
        assert np.array_equal(got_frames[0] + got_frames[1], want_frames)  # the two shards partition the grid
    finally:
        for sh in shards:
            sh.close()


def test_replay_and_epoch_wrap_under_a_mask(monkeypatch):
    monkeypatch.delenv("RENE_TEST_DROP", raising=False)
    monkeypatch.delenv("RENE_TEST_EPOCH", raising=False)
    r, s, classes = scheduled("cornell")
    with r:
        want = [r.download(l) for l in range(3)]
        assert r.stats().launches == 3
    assert_tiles_equal_uniform("cornell", want, classes, s.xres, s.yres)
    monkeypatch.setenv("RENE_TEST_DROP", "2")  # the second launch drops one item in 97 (in software), and is launched again under its own mask
    r, _, _ = scheduled("cornell")
    with r:
        got = [r.download(l) for l in range(3)]
        assert r.stats().launches > 3  # the replay took place
    monkeypatch.delenv("RENE_TEST_DROP")
    for l in range(3):
        assert np.array_equal(got[l], want[l]), l
    monkeypatch.setenv("RENE_TEST_EPOCH", str((1 << 22) - 1 - 2))  # the third launch is the first of the new epoch
    r, _, _ = scheduled("cornell")
    with r:
        got = [r.download(l) for l in range(3)]
        assert np.array_equal(r.tile_frames(), ar.class_frames(classes))
    for l in range(3):
        assert np.array_equal(got[l], want[l]), l


def test_the_schedule_end_to_end():
    s = scenes.cornell_box(192, 128)
    target, cap = 0.2, 64
    n_t = ar.tile_pixels(192, 128)
    with api.Renderer(s) as r:
        frames, est = r.render_adaptive(target=target, max_frames=cap, batch=16, dilate=0)
        layers = [r.download(l) for l in range(3)]
        st = r.stats().as_dict()
        assert np.array_equal(frames, r.tile_frames())
    print("dilate 0: N_t\n", frames, "\npaths", st["paths"], "of", cap * 192 * 128)
    assert frames.shape == (4, 6) and (frames == 16).sum() >= 4 and (frames == cap).sum() >= 4
    assert st["paths"] == int((frames.astype(np.int64) * n_t).sum()) < cap * 192 * 128
    assert est.n_frames == frames.max() == st["frames"]
    with api.Renderer(s) as u:  # uniform renders at every N_t that occurs
        for n in np.unique(frames):
            u.reset()
            u.render(0, int(n))
            ref = [u.download(l) for l in range(3)]
            e = u.estimate_noise()
            tn = np.sqrt(ar.tile_q(*(u.noise_tiles()[k] for k in ("sum_var", "sum_lum", "n_pixels")), e.luminance_floor))
            for t, sl in ar.tile_slices(192, 128):
                if frames[t] != n:
                    continue
                for l in range(3):
                    assert np.array_equal(layers[l][sl], ref[l][sl]), (t, int(n), l)
                if n < cap:
                    assert tn[t] <= target, (t, int(n), float(tn[t]))  # it stopped because it had met the target
    with api.Renderer(s) as r:
        wider, _ = r.render_adaptive(target=target, max_frames=cap, batch=16, dilate=1)
    print("dilate 1: N_t\n", wider)
    assert (wider >= frames).all()


def _code(call):
    with pytest.raises(api.ReneError) as e:
        call()
    assert str(e.value).split(": ", 1)[1].strip()  # a non-empty rene_last_error
    return e.value.code


def test_refusals():
    s = scenes.cornell_box(96, 64)
    classes = ar.tile_classes(96, 64)
    with api.Renderer(s) as r:
        r.set_active_tiles(None)  # all active: nothing to do
        r.render(0, 16)
        r.denoise()
        r.set_active_tiles(classes != "A")
        assert _code(lambda: r.set_active_tiles(np.ones(classes.shape))) == -1   # re-activation
        assert _code(lambda: r.set_active_tiles(None)) == -1                      # ... by NULL too
        assert _code(lambda: r.render(8, 8)) == -1                                # not where the context stands
        assert _code(lambda: r.render(24, 8)) == -1
        r.denoise()                                                               # tiles switched off, but every N_t is still 16
        r.render(16, 8)
        assert _code(lambda: r.denoise()) == -4                                   # uneven tiles
        assert np.array_equal(r.tile_frames(), np.where(classes == "A", 16, 24))
        r.set_active_tiles(np.zeros(classes.shape))
        before = r.stats().as_dict()
        r.render(24, 8)                                                           # no tile active: RENE_OK, no launch, nothing counted
        r.render(100, 8)
        after = r.stats().as_dict()
        assert after["launches"] == before["launches"] == 2 and after["frames"] == 24 and after["paths"] == before["paths"]
        r.reset()
        assert not r.tile_frames().any()
        r.render(0, 16)
        r.denoise()                                                               # works again
        assert (r.tile_frames() == 16).all() and r.stats().paths == 16 * 96 * 64
        r.set_active_tiles(np.ones(classes.shape))                                # every tile is active again after the reset
        r.render(40, 8)                                                           # (no mask: any frame range)
        assert _code(lambda: r.set_active_tiles(classes != "A")) == -1            # the frames so far are not one range
        assert _code(lambda: lib_set(r, classes, 3)) == -1                        # fewer entries than the grid has tiles
    with api.Renderer(scenes.dragon_class(96, 64, 20, 22), flags=abi.FLAG_WAVEFRONT) as w:
        assert _code(lambda: w.set_active_tiles(classes != "A")) == -4
    with api.Renderer(s, shard_mode=abi.SHARD_FRAMES, shard_rank=0, shard_count=2) as f:
        assert _code(lambda: f.set_active_tiles(classes != "A")) == -4
    with api.Renderer(s, shard_mode=abi.SHARD_FRAMES, shard_rank=0, shard_count=1) as f:  # a frame "shard" of one is an unsharded context
        f.set_active_tiles(classes != "A")


def lib_set(r, classes, n):
    a = np.ascontiguousarray(classes != "A", dtype=np.uint8)
    api._check(api.lib().rene_set_active_tiles(r._h, a.ctypes.data_as(api.C.c_void_p), n))
