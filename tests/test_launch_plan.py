"""CPU: the arithmetic of a render launch (rene_amd/csrc/launch_plan.h) -- a frame shard's share of a request, the cut of a chain's frames into
work items, the batches the work ids are handed out in -- against recorded results.

Every image is bit-identical however a job is cut (test_gpu_scenes.py), so the bit-identity suite cannot see a changed cut; only a slower job
would show it.  tests/golden/launch_plans.txt holds what the arithmetic gave while it was still part of rene_render, for a case list that takes
every branch of it (selftest/launch_plan_dump.cpp): a change of the tuned numbers has to change that file too, in the open."""
import os
import re
import subprocess

from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "rene_amd", "csrc")
DUMP = os.path.join(CSRC, "selftest", "launch_plan_dump")


def _block_size() -> int:
    """what render_block_size() returns (kernels.hip: BLOCK), read from the kernel unit's source"""
    assert "int render_block_size() { return BLOCK; }" in open(os.path.join(CSRC, "kernels.hip")).read()
    m = re.search(r"^constexpr int BLOCK = (\d+);", open(os.path.join(CSRC, "device_code.inc")).read(), re.M)
    assert m, "device_code.inc no longer defines BLOCK as a literal"
    return int(m.group(1))


def test_launch_plans_are_the_recorded_ones(hip_lib):
    if not os.path.exists(DUMP):  # (the library was built by hand: `make` builds this with it)
        subprocess.check_call(["make", "-C", CSRC, "selftest/launch_plan_dump"])
    got = subprocess.run([DUMP, str(_block_size())], check=True, capture_output=True, text=True).stdout.splitlines()
    want = open(os.path.join(GOLDEN, "launch_plans.txt")).read().splitlines()
    assert len(want) >= 300 and {line.split()[0] for line in want} == {"share", "cut", "batch"}
    # the inputs are part of every line: a case list that changed without the fixture shows here, not as a wall of differences
    assert [g.split(" -> ")[0] for g in got] == [w.split(" -> ")[0] for w in want], "the case list and the fixture differ"
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(want)} plans changed; the first (got, recorded): {wrong[0]}"
