"""The renders of the prepared-path-start parity test (test_gpu_start_slot.py) and of the tool that records its fixtures
(tests/golden/make_start_slot_fixtures.py): the smallest jobs in which a path start prepared for the wrong pixel, the wrong frame or the wrong
item shows, through the Matte small-scene kernels whose path start csrc/device_code.inc prepares ahead (RENE_START_SLOT)."""
import contextlib
import json
import os

import numpy as np

from emit_fusion_scenes import cornell_sun
from rene_amd import abi, api, scenes

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "start_slot")
TIMINGS = ("kernel_ms", "last_launch_ms", "sclk_mhz")  # measured per launch: never equal between two renders

SMALL = lambda: scenes.cornell_box(40, 24)
# tiles of the 2 x 2 grid of a 64 x 64 film that stay active in the adaptive case's second call
SOME_OFF = np.array([[1, 0], [0, 1]], np.uint8)

# name: (scene, [(first_frame, n_frames), ...] render calls, Renderer options, environment, active tiles or None)
CASES = {
    # nineteen frames over the eight chains are 3, 3, 3, 2, 2, 2, 2, 2: the lanes of a wave run out of frames -- and of starts to prepare -- at
    # different times, and take their next item at different times
    "one-launch": (SMALL, [(0, 19)], {}, {}, None),
    "two-launches": (SMALL, [(0, 7), (7, 12)], {}, {}, None),  # chains of 0 - 1 and of 1 - 2 frames; the second launch continues the first
    # partial tiles, and lanes that never get an item: their slot stays empty and is never read
    "shard-1-of-3": (lambda: scenes.cornell_box(33, 33), [(0, 19)], {"shard_mode": abi.SHARD_TILES, "shard_rank": 1, "shard_count": 3}, {}, None),
    "cornell-sun": (lambda: cornell_sun(40, 24), [(0, 19)], {}, {}, None),  # FEAT_LIGHTS | FEAT_SMALL: the <72, ...> kernels
    "drop-replay": (SMALL, [(0, 19)], {}, {"RENE_TEST_DROP": "1"}, None),  # one item in 97 dropped: the host's replay, ITEM_DONE
    # the second call's items of the switched-off tiles are empty (frame = frame_end): nothing to prepare, and nothing prepared may be left over
    "tiles-off": (lambda: scenes.cornell_box(64, 64), [(0, 8), (8, 8)], {}, {}, SOME_OFF),
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
