"""CPU: the item-length policy of the small-scene jobs (rene_amd/csrc/launch_plan.h, small_scene_item_frames) and what item_cut makes of its
answer (selftest/tail_cut_dump.cpp prints both, with the untuned cut beside them).  The policy moves frames from a job's last item to its first
and nothing else: for every input the levels' frames sum to F, there are never more levels than the untuned cut has, and the last item is never
longer than the first; outside what was measured (profiles/tail_cut_ab.txt) it answers 0, the untuned cut."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "rene_amd", "csrc")
DUMP = os.path.join(CSRC, "selftest", "tail_cut_dump")

FS = (1, 4, 63, 64, 65, 127, 128, 129, 512, 1024, 8192)
PIXELS = (1024, 131072, 1 << 20, 2 << 20, 1 << 23)
MI355X_LANES = 256 * 8 * 256  # the persistent launch's upper bound there: 8 workgroups of 256 lanes per compute unit
LANES = (MI355X_LANES, 64 * 8 * 256, 0)  # ... a quarter of the chip, and no lanes at all


@pytest.fixture(scope="module")
def answers(hip_lib):
    if not os.path.exists(DUMP):  # (the library was built by hand: `make` builds this with it)
        subprocess.check_call(["make", "-C", CSRC, "selftest/tail_cut_dump"])
    cases = [(F, px, lanes) for lanes in LANES for px in PIXELS for F in FS]
    out = subprocess.run([DUMP], input="".join(f"{F} {px} {lanes}\n" for F, px, lanes in cases), check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(cases)
    got = {}
    for case, line in zip(cases, out):
        m = re.fullmatch(r"F=(\d+) owned_pixels=(\d+) lanes=(\d+) -> item_frames=(\d+) levels=([\d,]+) untuned=([\d,]+)", line)
        assert m and tuple(int(m.group(i)) for i in (1, 2, 3)) == case, line
        got[case] = (int(m.group(4)), [int(x) for x in m.group(5).split(",")], [int(x) for x in m.group(6).split(",")])
    return got


def test_the_cut_keeps_the_frames_and_adds_no_level(answers):
    for (F, px, lanes), (item, levels, untuned) in answers.items():
        assert sum(levels) == F and sum(untuned) == F, (F, px, lanes)
        assert len(levels) <= len(untuned), (F, px, lanes)
        assert levels[-1] <= levels[0] and min(levels) >= 1, (F, px, lanes)
        if item == 0:
            assert levels == untuned, (F, px, lanes)
        else:
            assert levels == [item, F - item] and F - item < item, (F, px, lanes)


def test_the_policy_is_zero_outside_the_measured_domain(answers):
    # measured with a gain, on the MI355X: F from 128 to 512 on the whole 2^20-pixel image; nothing else (an eighth of its tiles gained nothing)
    for F in FS:
        for px in PIXELS:
            inside = px == 1 << 20 and 128 <= F <= 512
            assert (answers[(F, px, MI355X_LANES)][0] != 0) == inside, (F, px)
    # whatever the lanes: no image beyond 2^20 pixels, none as small as 1024, no F outside 128 .. 512, and nothing without lanes
    assert all(answers[(F, px, 0)][0] == 0 for F in FS for px in PIXELS)
    assert all(answers[(F, px, lanes)][0] == 0 for F in FS for px in (1024, 2 << 20, 1 << 23) for lanes in LANES)
    assert all(answers[(F, px, lanes)][0] == 0 for F in FS if F < 128 or F > 512 for px in PIXELS for lanes in LANES)


def test_the_policy_inside_it(answers):
    assert answers[(128, 1 << 20, MI355X_LANES)][:2] == (112, [112, 16])  # the bench job: F / 8
    assert answers[(129, 1 << 20, MI355X_LANES)] == (113, [113, 16], [64, 64, 1])  # an odd F: two levels where the untuned cut has three
    assert answers[(512, 1 << 20, MI355X_LANES)][:2] == (448, [448, 64])
    assert answers[(128, 131072, MI355X_LANES)][0] == 0  # one rank's eighth of the tiles, 2 items of a level per lane: the untuned cut
    # the bound is in items of a level per lane: on a quarter of the lanes the eighth share has 8 per lane (still too few), the whole image 64
    assert answers[(128, 131072, LANES[1])][0] == 0 and answers[(128, 1 << 20, LANES[1])][0] == 112
