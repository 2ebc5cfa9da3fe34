"""The renders of the bounce-trim parity test (test_gpu_bounce_trims.py) and of the tool that records its fixtures
(tests/golden/make_bounce_trim_fixtures.py): small jobs through the Matte small-scene kernels whose bounce csrc/device_code.inc rearranges
(RENE_BOUNCE_TRIMS: the shared normalised ray, the branch-free shading frame, the static Matte BSDF), and one kernel that must not notice."""
import json
import os

import numpy as np

from emit_fusion_scenes import block_light, cornell_sun, deep_paths, triangle_light
from rene_amd import abi, api, scenes
from rene_amd.scene import TriangleMesh

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bounce_trims")
TIMINGS = ("kernel_ms", "last_launch_ms", "sclk_mhz")  # measured per launch: never equal between two renders

S = float(np.float32(np.sqrt(0.5)))  # both components of a diagonal normal are this one float: they stay equal through every normalize


def _diagonal_wall(p, n):
    """Cornell with one more Matte quad (the back wall's material) whose four vertex normals are n"""
    s = scenes.cornell_box(33, 17)
    back = s.instances[2].material_index
    s.add_triangle_mesh(TriangleMesh.from_arrays(p, [0, 1, 2, 0, 2, 3], normals=[n] * 4, uvs=[0, 0, 1, 0, 1, 1, 0, 1]), back)
    return s


def wall_about_vertical():
    """The back wall turned 45 degrees about the vertical, across the room's back left corner: shading normals with |n.x| == |n.z|"""
    return _diagonal_wall([-1, 0, 0.2, -1, 2, 0.2, 0.2, 2, -1, 0.2, 0, -1], (S, 0.0, S))


def wall_about_view_axis():
    """The same wall turned 45 degrees about the view axis, across the corner of the left wall and the floor: |n.x| == |n.y|, the tie of the
    shading frame's test (onb_from_w: |w.x| > |w.y| is false, the second form)"""
    return _diagonal_wall([-1, 1.2, -1, -1, 1.2, 1, 0.2, 0, 1, 0.2, 0, -1], (S, S, 0.0))


# name: (scene, frames, Renderer options)
CASES = {
    "deep-paths": (lambda: deep_paths(32, 32), 8, {}),  # roulette beyond depth 12, the deferred one included
    "triangle-light": (lambda: triangle_light(40, 24), 16, {}),  # a twin triangle: the emitter query answered behind the next loop
    "block-light": (lambda: block_light(40, 24), 16, {}),  # no twin: the separate emitter query, with its own normalize of the new ray
    "cornell-sun": (lambda: cornell_sun(40, 24), 16, {}),  # FEAT_LIGHTS | FEAT_SMALL
    "wall-vertical": (wall_about_vertical, 16, {}),
    "wall-view-axis": (wall_about_view_axis, 16, {"flags": abi.FLAG_COUNTERS}),  # the counting instantiation
    "veach-mis": (lambda: scenes.veach_mis(40, 24), 8, {}),  # Matte + Metal, spheres: a kernel the trims are not enabled in
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
