"""Test helper (not a conftest): the scenes of the light-group pass's tests (rene_lights, include/rene_hip.h) and the BLACKING of their sources.

`cornell()` is the Cornell box at 72 x 40 -- a partial tile column and a partial tile row, so the clamped dead lanes run -- with its ceiling light,
a second emitting quad on the left wall and one distant light: all Matte, the item loop unless FLAG_FORCE_BVH.  `zoo()` is the material zoo at the
size tests/test_gpu_direct.py uses: a background with a texture, one distant light, a triangle emitter and a sphere emitter, the general form.
`deep()` is tests/emit_fusion_scenes.py's deep_paths(32, 32).

`default_groups(scene)` is the library's grouping of a scene's sources (rene_lights_default_groups, restated here): group 0 the background, then a
group per distant light in table order, then one per instance with an area light in instance order, the overflow in group 7.  `only(builder, g)`
builds the scene again with every source OUTSIDE group g black: the radiance of an area light, of a distant light, the background colour set to
zero, each source left in its table.  scene_pack.cpp decides "emitter" by the area light's type and keeps every distant light, so the emitter
structure, the mixture, every draw and every throughput are the full scene's; a black background drops FEAT_BACKGROUND, which in a scene that stays
general for other reasons (the zoo: textures, general materials) only turns the miss add into the + 0 it would have been anyway.  `scaled(builder,
g, k)` multiplies the radiance of group g's sources by k instead."""
import numpy as np

import emit_fusion_scenes
from rene_amd import abi, scenes
from rene_amd.scene import TriangleMesh

CORNELL_W, CORNELL_H = 72, 40
SUN = ((-0.18862, 0.692312, 0.69651), (0, 0, 0), (3, 3, 3))  # the direction tests/test_gpu_direct.py's Cornell sun has, dimmer


def cornell(w=CORNELL_W, h=CORNELL_H):
    s = scenes.cornell_box(w, h)
    lamp = s.add_area_light_diffuse((2.0, 6.0, 9.0))
    quad = TriangleMesh.from_arrays([-0.98, 0.6, -0.3, -0.98, 1.2, -0.3, -0.98, 1.2, 0.3, -0.98, 0.6, 0.3], [0, 1, 2, 0, 2, 3], normals=[(1, 0, 0)] * 4)
    s.add_triangle_mesh(quad, s.add_matte((0.0, 0.0, 0.0)), area_light=lamp)
    s.add_light_distant(*SUN)
    return s


def zoo():
    return scenes.material_zoo(96, 64)


def deep():
    return emit_fusion_scenes.deep_paths(32, 32)


def many_sources(w=32, h=32):
    """Ten sources -- no background, three distant lights, the Cornell box's lamp, the second one and four small ones on the floor -- for eight
    groups: the last three lamps share group 7."""
    s = cornell(w, h)
    s.add_light_distant((0.3, 0.9, 0.4), (0, 0, 0), (1, 2, 1))
    s.add_light_distant((-0.5, 0.4, 0.8), (0, 0, 0), (2, 1, 1))
    for k in range(4):
        x = -0.75 + 0.5 * k
        lamp = s.add_area_light_diffuse((4.0 + k, 5.0, 8.0 - k))
        quad = TriangleMesh.from_arrays([x, 0.01, 0.6, x, 0.01, 0.8, x + 0.2, 0.01, 0.8, x + 0.2, 0.01, 0.6], [0, 1, 2, 0, 2, 3], normals=[(0, 1, 0)] * 4)
        s.add_triangle_mesh(quad, s.add_matte((0.0, 0.0, 0.0)), area_light=lamp)
    return s


def default_groups(scene):
    """((instance_group, distant_group, background_group), n_used): rene_lights_default_groups restated."""
    nxt = 1
    dist = np.zeros(len(scene.lights), np.uint8)
    inst = np.zeros(len(scene.instances), np.uint8)
    for li in range(len(scene.lights)):
        dist[li] = min(nxt, 7)
        nxt += 1
    for k, i in enumerate(scene.instances):
        if scene.area_lights[i.area_light_index].type != abi.AREA_LIGHT_NULL:
            inst[k] = min(nxt, 7)
            nxt += 1
    return (inst, dist, 0), min(nxt, 8)


def emitting(scene):
    return [k for k, i in enumerate(scene.instances) if scene.area_lights[i.area_light_index].type != abi.AREA_LIGHT_NULL]


def _scale_outside(scene, keep, k_in, k_out):
    """Multiply every source's radiance by k_in where its group is `keep` and by k_out elsewhere.  Area lights are shared by index: each emitting
    instance of these scenes has one of its own."""
    (inst, dist, bg), _ = default_groups(scene)
    lights_of = {}
    for k in emitting(scene):
        lights_of.setdefault(scene.instances[k].area_light_index, set()).add(int(inst[k]))
    for al, groups in lights_of.items():
        assert len(groups) == 1
        f = k_in if groups == {keep} else k_out
        for c in range(3):
            scene.area_lights[al].v0[c] *= f
    for li, l in enumerate(scene.lights):
        f = k_in if int(dist[li]) == keep else k_out
        for c in range(3):
            l.v1[c] *= f
    f = k_in if bg == keep else k_out
    scene.background_color = tuple(float(np.float32(c) * np.float32(f)) for c in scene.background_color)
    return scene


def only(builder, g):
    """The builder's scene with every source outside group g black."""
    return _scale_outside(builder(), g, 1.0, 0.0)


def scaled(builder, g, k):
    """The builder's scene with the radiance of group g's sources times k (a power of two keeps every product exact)."""
    return _scale_outside(builder(), g, float(k), 1.0)
