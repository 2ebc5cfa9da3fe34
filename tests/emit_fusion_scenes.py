"""Scenes of the emitter-query fusion tests (test_emit_fusion.py, test_gpu_emit_fusion.py): which main item the packer marks as the emitter
structure's twin (csrc/scene_pack.cpp, mark_emit_twin), read back through rene_scene_small_items."""
import numpy as np

from rene_amd import abi, api, scenes
from rene_amd.scene import TriangleMesh

SUN = ((-0.18862, 0.692312, 0.69651), (0, 0, 0), (8, 8, 8))


def cornell_sun(w, h):
    s = scenes.cornell_box(w, h)
    s.add_light_distant(*SUN)
    return s


def _replace_light(s, mesh):
    light = s.instances[-1]  # the light quad (the last instance)
    material, area = light.material_index, light.area_light_index
    s.instances.pop()
    s.add_triangle_mesh(mesh, material, area_light=area)
    return s


def triangle_light(w, h):
    """Cornell lit by ONE triangle: the emitter structure's only item is a TRIANGLE item, and so is its twin."""
    tri = TriangleMesh.from_arrays([-0.24, 1.98, -0.22, 0.23, 1.98, -0.22, 0.23, 1.98, 0.16], [0, 1, 2], normals=[(0, -1, 0)] * 3,
                                   uvs=[0, 0, 1, 0, 1, 1])
    return _replace_light(scenes.cornell_box(w, h), tri)


def block_light(w, h):
    """Cornell whose light quad is the lower face of a closed emissive block: both structures merge the six faces into one BOX item."""
    return _replace_light(scenes.cornell_box(w, h), scenes._aabb((-0.24, 1.98, -0.22), (0.23, 1.995, 0.16)))


def deep_paths(w=32, h=32):
    """Cornell with every Matte reflectance, the light's included, at 0.95: paths run long, so the roulette beyond depth 12 and the depth
    cap decide real lanes (the CPU oracle: 954 of this scene's 127 893 rays at 16 frames lie beyond depth 13; plain Cornell has 59 in 323 k)."""
    s = scenes.cornell_box(w, h)
    for t in s.textures:
        if t.type == abi.TEXTURE_SOLID:
            t.v0[0:3] = [0.95, 0.95, 0.95]
    return s


def twin_marks(scene):
    """(indices of the main loop items marked SMALL_ITEM_EMIT_TWIN, main records, main loop length, emitter records, emitter loop length)"""
    main, n_main = api.small_items(scene, 0)
    emit, n_emit = api.small_items(scene, 1)
    marked = [int(i) for i in np.nonzero(main[:n_main, 15] & abi.SMALL_ITEM_EMIT_TWIN)[0]]
    assert not (emit[:, 15] & abi.SMALL_ITEM_EMIT_TWIN)[:n_emit].any()  # the emitter structure's own items are never marked
    return marked, main, n_main, emit, n_emit
