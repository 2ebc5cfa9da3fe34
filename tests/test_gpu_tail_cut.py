"""The cut of a small-scene job into a long first item and a short last one (launch_plan.h, small_scene_item_frames, in front of item_cut;
DESIGN.md section 4, profiles/tail_cut_ab.txt) changes when a chain's frames are rendered, never what is computed: the same frames in the same
order, so the three layers and every counter of rene_stats are those of any other cut.  The default is held against today's two equal items,
against the policy's own cuts brought in through the knob, and against RENE_FLAG_SINGLE_LEVEL, on a film ragged in both directions."""
import numpy as np
import pytest

import item_switch_cases as cases
from emit_fusion_scenes import cornell_sun
from rene_amd import abi, api, scenes


def _render(build, calls, opts=None, env=None):
    """(layers [3, H, W, 3] float32 sums, the counters of rene_stats without the timings)"""
    with cases._environment(env or {}), api.Renderer(build(), **(opts or {})) as r:
        for first, n in calls:
            r.render(first, n)
        r.sync()
        layers = np.stack([r.download(k) for k in range(3)])
        st = {k: int(v) for k, v in r.stats().as_dict().items() if k not in cases.TIMINGS}
    return layers, st


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == np.float32
    for k in range(3):
        assert np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


# ---- the cut: 1024 frames in one launch, a chain's share F = 128; a film ragged in both directions (40 x 24: two tiles, neither full) ----------------
CUT_SCENES = {"cornell": lambda: scenes.cornell_box(40, 24), "cornell-sun": lambda: cornell_sun(40, 24)}
# what the default is held against: today's two items of 64, the policy's cut for F = 128 (112 + 16) and a longer last item (96 + 32) through
# the knob -- a film this small lies outside the policy's domain, so the knob is what brings its cut here -- and one item per launch
CUT_OTHERS = {"items-64": ({}, {"RENE_ITEM_FRAMES": "64"}), "items-112": ({}, {"RENE_ITEM_FRAMES": "112"}), "items-96": ({}, {"RENE_ITEM_FRAMES": "96"}),
              "single-level": ({"flags": abi.FLAG_SINGLE_LEVEL}, {})}


@pytest.fixture(scope="module")
def cut_default():
    return {name: _render(build, [(0, 1024)]) for name, build in CUT_SCENES.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("other", list(CUT_OTHERS))
@pytest.mark.parametrize("scene", list(CUT_SCENES))
def test_the_cut_changes_neither_layers_nor_counters(cut_default, scene, other):
    layers, st = cut_default[scene]
    assert layers[0].any() and st["paths"] == 40 * 24 * 1024
    opts, env = CUT_OTHERS[other]
    got, st2 = _render(CUT_SCENES[scene], [(0, 1024)], opts, env)
    _same(layers, got, (scene, other))
    assert st == st2, (scene, other)
