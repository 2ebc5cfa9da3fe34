"""The renders of the work-item switch parity test (test_gpu_item_switch.py) and of the tool that records its fixtures
(tests/golden/make_item_switch_fixtures.py): the smallest jobs in which a wrong pixel slot or a wrong tile shows, through the Matte small-scene
kernels whose item bookkeeping csrc/device_code.inc changes (RENE_ITEM_SWITCH: the lane keeps its slot), and one kernel that must not notice."""
import contextlib
import json
import os

import numpy as np

from emit_fusion_scenes import cornell_sun
from rene_amd import abi, api, scenes

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "item_switch")
TIMINGS = ("kernel_ms", "last_launch_ms", "sclk_mhz")  # measured per launch: never equal between two renders

RAGGED = lambda: scenes.cornell_box(100, 70)  # 4 x 3 tiles, ragged in both directions
SHARD_1_OF_3 = {"shard_mode": abi.SHARD_TILES, "shard_rank": 1, "shard_count": 3}  # owned tile k is image tile 1 + 3 k: across the tile rows
# tiles of the 3 x 4 grid that stay active: one off in every row and column, the ragged corner among them
SOME_OFF = np.array([[1, 0, 1, 1], [1, 1, 0, 1], [0, 1, 1, 0]], np.uint8)

# name: (scene, [(first_frame, n_frames), ...] render calls, Renderer options, environment, active tiles or None)
CASES = {
    # 21 frames over the eight chains are 3, 3, 3, 3, 3, 2, 2, 2: three levels of one frame each -- the last item of three chains is empty, and
    # every level hands off to the next
    "ragged-levels": (RAGGED, [(0, 21)], {}, {"RENE_LEVELS": "3"}, None),
    "shard-two-calls": (RAGGED, [(0, 16), (16, 8)], SHARD_1_OF_3, {}, None),  # the second launch continues from prev_final
    "cornell-sun": (lambda: cornell_sun(40, 24), [(0, 16)], {}, {}, None),  # FEAT_LIGHTS | FEAT_SMALL: the <72, ...> kernels
    "tiles-off": (RAGGED, [(0, 8), (8, 8)], {}, {}, SOME_OFF),  # the second call's items of the switched-off tiles are empty
    "drop-replay": (RAGGED, [(0, 16)], {}, {"RENE_TEST_DROP": "1"}, None),  # one item in 97 dropped: the replay, ITEM_DONE
    "counters": (RAGGED, [(0, 16)], {"flags": abi.FLAG_COUNTERS}, {}, None),  # the counting instantiation
    "veach-mis": (lambda: scenes.veach_mis(40, 24), [(0, 8)], {}, {}, None),  # Matte + Metal, spheres: a kernel the predicate leaves alone
}
KNOBS = ("RENE_LEVELS", "RENE_TEST_DROP", "RENE_ITEM_FRAMES", "RENE_ITEM_TAIL", "RENE_WORK_BATCH")


@contextlib.contextmanager
def _environment(env):
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def render_case(name):
    """(layers [3, H, W, 3] float32, the counters of rene_stats without the timings)"""
    build, calls, opts, env, active = CASES[name]
    with _environment(env), api.Renderer(build(), **opts) as r:
        for i, (first, n) in enumerate(calls):
            if active is not None and i == len(calls) - 1:
                r.set_active_tiles(active)
            r.render(first, n)
        r.sync()
        layers = np.stack([r.download(k) for k in range(3)])
        st = {k: int(v) for k, v in r.stats().as_dict().items() if k not in TIMINGS}
    return layers, st


def layers_path(name, directory=DIR):
    """the case's three layers, one compressed file: [3, H, W, 3] float32 under the key `layers`"""
    return os.path.join(directory, f"{name}.npz")


def load_counters(directory=DIR):
    with open(os.path.join(directory, "counters.json")) as f:
        return json.load(f)
