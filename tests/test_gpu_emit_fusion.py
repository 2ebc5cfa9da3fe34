"""The emitter query answered inside the next bounce's closest-hit loop (csrc/device_code.inc, EmitCapture).

One library renders both ways: RENE_EMIT_FUSION=0, read when a scene is packed, marks no item and the kernels run the separate emitter query
of every bounce as before.  What is checked: fusion on against fusion off -- the three layers EQUAL and every counter of rene_stats equal (the
timings of a launch aside) -- over the configurations in CASES; fusion off against the layers recorded before the fusion existed
(tests/golden/frame_stream_layers.npz); and a scene of long paths, where the deferred roulette and the depth cap decide lanes, against the CPU
oracle."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from emit_fusion_scenes import cornell_sun, deep_paths, triangle_light, twin_marks
from rene_amd import abi, api, scenes
from test_gpu_frame_stream import many_emitters

W, H, FRAMES, SPLIT = 48, 40, 16, 9
TIMINGS = ("kernel_ms", "last_launch_ms", "sclk_mhz")  # measured per launch: never equal between two renders


def render(monkeypatch, scene, fusion, flags=0, calls=((0, FRAMES),), **opts):
    if fusion is None:
        monkeypatch.delenv("RENE_EMIT_FUSION", raising=False)
    else:
        monkeypatch.setenv("RENE_EMIT_FUSION", "1" if fusion else "0")
    with api.Renderer(scene, flags=flags, **opts) as r:
        for first, n in calls:
            r.render(first, n)
        layers = np.stack([r.download(k) for k in range(3)])
        st = {k: v for k, v in r.stats().as_dict().items() if k not in TIMINGS}
    return layers, st, len(twin_marks(scene)[0])


CASES = {
    "cornell-aov": (lambda: scenes.cornell_box(W, H), {}),
    "cornell-noaov": (lambda: scenes.cornell_box(W, H), {"flags": abi.FLAG_NO_AOV}),
    "cornell-sun": (lambda: cornell_sun(W, H), {}),  # shadow queries run the same item list: they must capture nothing
    "cornell-sun-noaov": (lambda: cornell_sun(W, H), {"flags": abi.FLAG_NO_AOV}),
    "cornell-sun-split": (lambda: cornell_sun(W, H), {"calls": ((0, SPLIT), (SPLIT, FRAMES - SPLIT))}),
    "cornell-sun-shard": (lambda: cornell_sun(W, H), {"shard_mode": abi.SHARD_TILES, "shard_rank": 1, "shard_count": 2}),
    "cornell-counters": (lambda: scenes.cornell_box(W, H), {"flags": abi.FLAG_COUNTERS}),
    "cornell-sun-counters": (lambda: cornell_sun(W, H), {"flags": abi.FLAG_COUNTERS}),
    "triangle-light": (lambda: triangle_light(W, H), {}),
    "triangle-light-counters": (lambda: triangle_light(W, H), {"flags": abi.FLAG_COUNTERS}),
    "deep-paths": (lambda: deep_paths(32, 32), {}),
    "deep-paths-counters": (lambda: deep_paths(32, 32), {"flags": abi.FLAG_COUNTERS}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_fusion_on_equals_fusion_off(monkeypatch, name):
    build, kw = CASES[name]
    on, st_on, marks_on = render(monkeypatch, build(), True, **kw)
    off, st_off, marks_off = render(monkeypatch, build(), False, **kw)
    assert (marks_on, marks_off) == (1, 0)  # the two renders did differ in what the kernel was told
    assert on[0].any() and st_on["rays_emitter"] > 0
    for k in range(3):
        assert np.array_equal(on[k], off[k]), (name, k, float(np.abs(on[k] - off[k]).max()))
    assert st_on == st_off, (name, st_on, st_off)
    if "counters" in name:
        assert st_on["prim_tests"] > 0


@pytest.mark.gpu
def test_a_scene_that_never_fuses_ignores_the_switch(monkeypatch):
    scene = many_emitters()[0]
    unset, st_unset, marks = render(monkeypatch, scene, None, calls=((3, 8),))
    off, st_off, _ = render(monkeypatch, scene, False, calls=((3, 8),))
    assert marks == 0 and np.array_equal(unset, off) and st_unset == st_off


@pytest.mark.gpu
@pytest.mark.parametrize("flags", ["aov", "noaov"])
@pytest.mark.parametrize("name", ["cornell", "cornell_sun"])
def test_fusion_off_equals_the_recorded_layers(monkeypatch, name, flags):
    """The fall-back path of this library against the layers of test_gpu_frame_stream.py (which holds the default, fused, path to them)."""
    want = np.load(os.path.join(GOLDEN, "frame_stream_layers.npz"))[f"{name}_{flags}"]
    scene = scenes.cornell_box(W, H) if name == "cornell" else cornell_sun(W, H)
    got, _, marks = render(monkeypatch, scene, False, flags=abi.FLAG_NO_AOV if flags == "noaov" else 0)
    assert marks == 0 and np.array_equal(got, want), (name, flags, float(np.abs(got - want).max()))


@pytest.mark.gpu
def test_deep_paths_render_against_the_oracle(monkeypatch, oracle_mod):
    """Long paths against the CPU oracle, the bounds of test_many_emitters_render_against_the_oracle: bad pixels <= 1e-3, relMSE <= 1e-4,
    paths equal -- fused (the default) and with the separate query."""
    scene = deep_paths(32, 32)
    o = oracle_mod.Oracle(scene)
    o.render(0, FRAMES)
    ref = o.download(0)
    so = o.stats().as_dict()
    for fusion in (None, False):
        layers, st, marks = render(monkeypatch, scene, fusion)
        gpu = layers[0]
        bad = (np.abs(gpu - ref) > 1e-2 * (1 + np.abs(ref))).any(axis=-1).mean()
        relmse = float(((gpu - ref) ** 2).sum() / (ref ** 2).sum())
        print(f"deep paths against the oracle, fusion {'on' if fusion is None else 'off'}: bad pixels {bad:.3g}, relMSE {relmse:.3g}, "
              f"rays {st['rays_closest'] + st['rays_shadow'] + st['rays_emitter']} (oracle {so['rays']})")
        assert marks == (1 if fusion is None else 0)
        assert bad <= 1e-3 and relmse <= 1e-4, (fusion, bad, relmse)
        assert st["paths"] == so["paths"]
