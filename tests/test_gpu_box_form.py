"""The box item's test in the closest-hit loop of the Matte small-scene kernels (csrc/box_slabs.h) computes what
the loop computed before it was rewritten: the three layers and every counter of the renders in box_form_cases.py, byte for byte, against
fixtures recorded with the build of the commit before (tests/golden/make_box_form_fixtures.py, tests/golden/box_form/)."""
import os

import numpy as np
import pytest

import box_form_cases as cases



@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.CASES))
def test_layers_and_counters_are_the_recorded_ones(name):
    layers, counters = cases.render_case(name)
    assert layers[0].any() and counters["paths"] > 0
    if "counters" in name:
        assert counters["prim_tests"] > 0
    for k in range(3):
        want = np.load(cases.layer_path(name, k))
        assert want.dtype == np.float32 and want.shape == layers[k].shape
        same = layers[k].view(np.uint32) == want.view(np.uint32)  # the bits: -0 is not +0 here, and a NaN equals itself
        assert same.all(), (name, k, int((~same).sum()), float(np.nanmax(np.abs(layers[k] - want))))
    assert counters == cases.load_counters()[name], name


def test_the_fixtures_are_all_there():  # CPU
    assert sorted(os.listdir(cases.DIR)) == sorted([f"{n}_layer{k}.npy" for n in cases.CASES for k in range(3)] + ["counters.json"])
