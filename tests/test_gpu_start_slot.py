"""The path start of the Matte small-scene kernels, prepared ahead (csrc/device_code.inc, RENE_START_SLOT) -- a lane keeps
one prepared primary ray in LDS and the start block runs for every lane of the wave with an empty slot at once -- computes what the start computed
before: the three layers and every counter of rene_stats of the renders in start_slot_cases.py, byte for byte, against fixtures recorded with the
build of the commit before (tests/golden/make_start_slot_fixtures.py, tests/golden/start_slot/).  The cases are the smallest in which a start
prepared for the wrong frame or left over from another item shows: chains of two and three frames in one launch, the same frames in two launches,
a tile shard with partial tiles and lanes that never get an item, the kernels with a distant light, a dropped and replayed launch, tiles
switched off.

(The refill counters of the counting instantiation -- counters[19 .. 20], printed under RENE_DEBUG -- are not part of rene_stats and depend on
which wave takes which batch: they are measured in profiles/start_slot_ab.txt, not compared here.)"""
import os

import numpy as np
import pytest

import start_slot_cases as cases


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.CASES))
def test_layers_and_counters_are_the_recorded_ones(name):
    layers, counters = cases.render_case(name)
    assert layers[0].any() and counters["paths"] > 0
    want = np.load(cases.layers_path(name))["layers"]
    assert want.dtype == np.float32 and want.shape == layers.shape
    for k in range(3):
        same = layers[k].view(np.uint32) == want[k].view(np.uint32)  # the bits: -0 is not +0 here, and a NaN equals itself
        assert same.all(), (name, k, int((~same).sum()), float(np.nanmax(np.abs(layers[k] - want[k]))))
        assert np.array_equal(layers[k], want[k], equal_nan=True), (name, k)
    assert counters == cases.load_counters()[name], name


def test_the_fixtures_are_all_there():  # CPU
    assert sorted(os.listdir(cases.DIR)) == sorted([f"{n}.npz" for n in cases.CASES] + ["counters.json"])


def test_the_cases_are_what_they_claim():  # CPU
    assert sorted(len(range(g, 19, 8)) for g in range(8)) == [2, 2, 2, 2, 2, 3, 3, 3]  # nineteen frames: chains of two and of three
    off = cases.SOME_OFF
    assert off.shape == (2, 2) and (off == 0).any() and (off != 0).any()
    assert [sum(n for _, n in cases.CASES[c][1]) for c in ("one-launch", "two-launches")] == [19, 19]
