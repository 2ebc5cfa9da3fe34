"""The work-item switch of the Matte small-scene kernels (csrc/device_code.inc, RENE_ITEM_SWITCH) -- the lane keeps its
pixel slot instead of rebuilding it at every commit, load and poll -- computes what the bookkeeping computed before: the three layers and every counter of rene_stats of the renders in item_switch_cases.py,
byte for byte, against fixtures recorded with the build of the commit before (tests/golden/make_item_switch_fixtures.py,
tests/golden/item_switch/).  The cases are the smallest in which a wrong slot or tile shows: a film ragged in both directions, a tile shard whose
owned tiles lie across the tile rows, a second launch that continues from the first, levels with empty items, tiles switched off, a dropped and
replayed launch, the counting instantiation, the kernels with a distant light, and one kernel the change leaves alone.

(The pass and lane-state counters of the counting instantiation -- counters[12 .. 18], printed under RENE_DEBUG -- are not part of rene_stats and
depend on which wave takes which batch: they are measured in profiles/item_switch_ab.txt, not compared here.)"""
import os

import numpy as np
import pytest

import item_switch_cases as cases


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.CASES))
def test_layers_and_counters_are_the_recorded_ones(name):
    layers, counters = cases.render_case(name)
    assert layers[0].any() and counters["paths"] > 0
    if "flags" in cases.CASES[name][2]:
        assert counters["prim_tests"] > 0
    want = np.load(cases.layers_path(name))["layers"]
    assert want.dtype == np.float32 and want.shape == layers.shape
    for k in range(3):
        same = layers[k].view(np.uint32) == want[k].view(np.uint32)  # the bits: -0 is not +0 here, and a NaN equals itself
        assert same.all(), (name, k, int((~same).sum()), float(np.nanmax(np.abs(layers[k] - want[k]))))
    assert counters == cases.load_counters()[name], name


def test_the_fixtures_are_all_there():  # CPU
    assert sorted(os.listdir(cases.DIR)) == sorted([f"{n}.npz" for n in cases.CASES] + ["counters.json"])


def test_the_cases_are_what_they_claim():  # CPU
    chains = [len(range(g, 21, 8)) for g in range(8)]
    assert sorted(set(chains)) == [2, 3]  # RENE_LEVELS=3 on 21 frames: a third item that is empty for the chains with two
    off = cases.SOME_OFF
    assert off.shape == (3, 4) and (off == 0).any(axis=0).all() and (off == 0).any(axis=1).all() and off[2, 3] == 0
