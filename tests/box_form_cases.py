"""The renders of the box-item parity test (test_gpu_box_form.py) and of the tool that records its fixtures
(tests/golden/make_box_form_fixtures.py): small jobs through every kernel whose closest-hit loop tests a box item in one of the forms of
csrc/box_slabs.h, and one that must not notice."""
import json
import os

import numpy as np

from emit_fusion_scenes import cornell_sun
from rene_amd import abi, api, scenes

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_form")
TIMINGS = ("kernel_ms", "last_launch_ms", "sclk_mhz")  # measured per launch: never equal between two renders

# name: (scene, frames, Renderer options)
CASES = {
    "cornell-odd": (lambda: scenes.cornell_box(33, 17), 16, {}),  # lanes without a pixel, partial waves
    "cornell-odd-counters": (lambda: scenes.cornell_box(33, 17), 16, {"flags": abi.FLAG_COUNTERS}),  # the counting instantiation: prim_tests
    "cornell-shard0": (lambda: scenes.cornell_box(64, 48), 24, {"shard_mode": abi.SHARD_TILES, "shard_rank": 0, "shard_count": 2}),
    "cornell-shard1": (lambda: scenes.cornell_box(64, 48), 24, {"shard_mode": abi.SHARD_TILES, "shard_rank": 1, "shard_count": 2}),
    "cornell-sun": (lambda: cornell_sun(64, 48), 24, {}),  # a distant light: any-hit queries over the same items
    "veach-mis": (lambda: scenes.veach_mis(40, 24), 8, {}),  # Matte + Metal, spheres: a kernel the forms are not enabled in
}


def render_case(name):
    """(layers [3, H, W, 3] float32, the counters of rene_stats without the timings)"""
    build, frames, opts = CASES[name]
    with api.Renderer(build(), **opts) as r:
        r.render(0, frames)
        layers = np.stack([r.download(k) for k in range(3)])
        st = {k: int(v) for k, v in r.stats().as_dict().items() if k not in TIMINGS}
    return layers, st


def layer_path(name, k, directory=DIR):
    return os.path.join(directory, f"{name}_layer{k}.npy")


def load_counters(directory=DIR):
    with open(os.path.join(directory, "counters.json")) as f:
        return json.load(f)
