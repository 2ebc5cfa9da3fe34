"""GPU: the RENE_DEBUG lines of the `atrous` denoiser's entry points.  tools/denoise_tiles_cost.py, tools/denoise_robust_cost.py and
tools/denoise_shard_cost.py read their figures from these lines, so their wording is an interface: the lines of one fixed sequence of calls, every
time in them replaced by `#`, are compared with tests/golden/denoise_debug_log.txt, and the tools' regular expressions must still find their lines.

The library reads RENE_DEBUG call by call and writes to the process's stderr: the calls run in a fresh child process started with the variable."""
import os
import re
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "denoise_debug_log.txt")
W, H, FRAMES = 100, 70, 12  # 12 tiles, ragged on both edges, chains of 2 and 1 frames (the smallest case of test_gpu_denoise_shards.py)


def child():
    sys.path.insert(0, ROOT)
    from rene_amd import abi, api, scenes
    make = lambda: scenes.cornell_box(W, H)
    with api.Renderer(make()) as r:
        r.render(0, FRAMES)
        r.denoise()
        r.denoise_tiles()
        r.denoise(robust=True)
        r.denoise_tiles(robust=True)
        shards = [api.Renderer(make(), shard_mode=abi.SHARD_TILES, shard_rank=rank, shard_count=2) for rank in range(2)]
        try:
            for s in shards:
                s.render(0, FRAMES)
                s.denoise_shard_prepare()
            for s in shards:
                r.denoise_place_shard(s.denoise_shard_buffer())
            r.denoise_placed()
        finally:
            for s in shards:
                s.close()


def captured_lines(env=None):
    """The child's `[rene] denoise` lines, times replaced."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(env or os.environ, RENE_DEBUG="1"), stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return [re.sub(r"\d+\.\d+", "#", line) for line in p.stderr.splitlines() if line.startswith("[rene] denoise")]


# the tools' patterns, restated (the tools match them against the raw lines; a time is \S+ or part of .*, which `#` satisfies as well)
TOOL_PATTERNS = {
    # tools/denoise_tiles_cost.py: both calls' lines, told apart by group 1
    "denoise_tiles_cost": [r"\[rene\] denoise(, tile by tile,)? .*ms: (.*); total (\S+)"],
    # tools/denoise_robust_cost.py: the trim kernel's line, then a plain call's
    "denoise_robust_cost": [r"\[rene\] denoise, trimmed prepare .*ms: trim (\S+)", r"\[rene\] denoise .*ms: (.*); total (\S+)"],
    # tools/denoise_shard_cost.py: its packed prepare runs on a shard of one ("shard 0 of 1"); the shards prepared here are 0 and 1 of 2, so that
    # pattern is restated with this sequence's shard numbers -- the rest of it is the tool's
    "denoise_shard_cost": [r"\[rene\] denoise, tile by tile, .*ms: prepare (\S+),", r"\[rene\] denoise shard 0 of 2, .*ms: packed prepare (\S+)",
                           r"\[rene\] denoise shard 0 of 2 placed, .*ms: place (\S+)"],
}


def test_debug_log_lines_are_the_recorded_ones():
    lines = captured_lines()
    for line in lines:
        print(line)
    with open(FIXTURE) as f:
        want = f.read().splitlines()
    assert lines == want
    for tool, patterns in TOOL_PATTERNS.items():
        for pattern in patterns:
            assert any(re.match(pattern, line) for line in lines), (tool, pattern)
    # denoise_tiles_cost.py tells the two calls apart by its first group and splits the second into "name ms" parts: both kinds are there
    kinds = {bool(m.group(1)) for m in (re.match(TOOL_PATTERNS["denoise_tiles_cost"][0], line) for line in lines) if m}
    assert kinds == {False, True}


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
