"""The bounce of the Matte small-scene kernels without the work its result does not need (csrc/device_code.inc, RENE_BOUNCE_TRIMS; DESIGN.md
section 4a) computes what it computed before: the three layers and every counter of the renders in bounce_trim_cases.py, byte for byte, against
fixtures recorded with the build of the commit before (tests/golden/make_bounce_trim_fixtures.py, tests/golden/bounce_trims/).  CPU: the
packer's guarantee the static Matte BSDF builds on -- a scene gets FEAT_TEXTURES with its first texture that is not Solid, and without it no
Matte instance is left unresolved (rene_scene_pack_info refuses one that is)."""
import os

import numpy as np
import pytest

import bounce_trim_cases as cases
from rene_amd import abi, api, scenes

FEAT_TEXTURES = 4


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.CASES))
def test_layers_and_counters_are_the_recorded_ones(name):
    layers, counters = cases.render_case(name)
    assert layers[0].any() and counters["paths"] > 0
    if "flags" in cases.CASES[name][2]:
        assert counters["prim_tests"] > 0
    for k in range(3):
        want = np.load(cases.layer_path(name, k))
        assert want.dtype == np.float32 and want.shape == layers[k].shape
        same = layers[k].view(np.uint32) == want.view(np.uint32)  # the bits: -0 is not +0 here, and a NaN equals itself
        assert same.all(), (name, k, int((~same).sum()), float(np.nanmax(np.abs(layers[k] - want))))
    assert counters == cases.load_counters()[name], name


def test_the_fixtures_are_all_there():  # CPU
    assert sorted(os.listdir(cases.DIR)) == sorted([f"{n}_layer{k}.npy" for n in cases.CASES for k in range(3)] + ["counters.json"])


def test_the_diagonal_walls_tie_the_frames_test():  # CPU
    for build, equal in ((cases.wall_about_vertical, (0, 2)), (cases.wall_about_view_axis, (0, 1))):
        n = build().meshes[-1].vertices[:, 3:6]
        assert (n[:, equal[0]].view(np.uint32) == n[:, equal[1]].view(np.uint32)).all() and (n[:, equal[0]] != 0).all()


def _checkered_cornell(checker: bool):
    s = scenes.cornell_box(33, 17)
    a, b = s.add_texture_solid((0.8, 0.8, 0.8)), s.add_texture_solid((0.1, 0.1, 0.1))
    tex = s.add_texture_checkerboard(a, b, 4.0, 4.0) if checker else s.add_texture_solid((0.4, 0.4, 0.4))
    floor = s.materials[s.instances[0].material_index]
    assert floor.type == abi.MATERIAL_MATTE
    floor.u0[0] = tex
    return s


def test_one_checkerboard_matte_sets_feat_textures(hip_lib):  # CPU
    info = api.pack_info(_checkered_cornell(True))
    assert info.features & FEAT_TEXTURES


def test_solid_textures_leave_no_matte_instance_unresolved(hip_lib):  # CPU
    # pack_info runs the packer's own check: a Matte instance whose kd shortcut is not valid in a scene without FEAT_TEXTURES is refused
    info = api.pack_info(_checkered_cornell(False))
    assert not info.features & FEAT_TEXTURES and info.features == api.pack_info(scenes.cornell_box(33, 17)).features
