"""GPU: rene-hip --lights PREFIX [--lights-frames N] [--lights-mix W0,W1,...] on the Cornell .pbrt fixture at 72 x 40 -- a file per group in use and
the groups' names, equal to the Python calls bit for bit, and the re-mix equal to api.lights_mix."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rene_amd import api, loader
from test_gpu_direct_cli import PBRT, _read_pfm

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
W, H = 72, 40


def _loaded():
    loaded = loader.load_pbrt(PBRT)
    desc = loaded.desc  # the command line's override of the Film size: the projection's x axis rescaled to the new aspect, in fp32
    ratio = np.float32(np.float32(W) / np.float32(H)) / np.float32(np.float32(desc.xresolution) / np.float32(desc.yresolution))
    desc.uniform.projection_inv[0] = np.float32(np.float32(desc.uniform.projection_inv[0]) * ratio)
    desc.xresolution, desc.yresolution = W, H
    loaded.xres, loaded.yres = W, H
    return loaded


def _run(tmp_path, *args):
    return subprocess.run([CLI, PBRT, "--width", str(W), "--height", str(H), "--spp", "4", "--out", "o.png", *args], capture_output=True, text=True, cwd=tmp_path)


def test_the_command_line_writes_a_file_per_group_and_their_names(hip_lib, tmp_path):
    p = _run(tmp_path, "--lights", "l")
    assert p.returncode == 0, p.stderr
    with api.Renderer(_loaded()) as r:
        (inst, dist, bg), used = r.light_groups()
        rec = r.lights(0, 4)  # the default of --lights-frames is the job's --spp
    assert used == 2 and bg == 0 and dist.size == 0 and sorted(inst.tolist())[-2:] == [0, 1]  # the background and the box's one lamp
    assert sorted(os.listdir(tmp_path)) == ["l.group0.pfm", "l.group1.pfm", "l.groups.txt", "o.png"]
    assert "INFO light-group pass over frames 0 .. 3, 2 groups" in p.stderr
    for g in range(used):
        assert _read_pfm(tmp_path / f"l.group{g}.pfm").tobytes() == api.lights_group_mean(rec, g).tobytes(), g
    assert not api.lights_group_mean(rec, 0).any() and api.lights_group_mean(rec, 1).sum() > 0
    lamp = int(np.nonzero(inst == 1)[0][0])
    assert open(tmp_path / "l.groups.txt").read() == f"group 0: background\ngroup 1: instance {lamp}\n"


def test_the_mix_is_the_apis(hip_lib, tmp_path):
    p = _run(tmp_path, "--lights", "l", "--lights-frames", "2", "--lights-mix", "3,0.25")
    assert p.returncode == 0, p.stderr
    assert sorted(os.listdir(tmp_path)) == ["l.group0.pfm", "l.group1.pfm", "l.groups.txt", "l.mix.pfm", "l.mix.png", "o.png"]
    assert "INFO light-group pass over frames 0 .. 1, 2 groups" in p.stderr and "the mix" in p.stderr
    with api.Renderer(_loaded()) as r:
        rec = r.lights(0, 2)
    w = np.ones(8, np.float32)
    w[:2] = [3, 0.25]
    mixed = api.lights_mix(rec, w)
    assert _read_pfm(tmp_path / "l.mix.pfm").tobytes() == mixed.tobytes() and mixed.sum() > 0
    assert _read_pfm(tmp_path / "l.group1.pfm").tobytes() == api.lights_group_mean(rec, 1).tobytes()
    png = open(tmp_path / "l.mix.png", "rb").read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and png[16:26] == W.to_bytes(4, "big") + H.to_bytes(4, "big") + b"\x08\x02"  # 8-bit RGB
    import zlib
    at, idat = 8, b""
    while at < len(png):
        n, kind = int.from_bytes(png[at:at + 4], "big"), png[at + 4:at + 8]
        if kind == b"IDAT":
            idat += png[at + 8:at + 8 + n]
        at += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 3 * W)
    assert not rows[:, 0].any() and np.array_equal(rows[:, 1:].reshape(H, W, 3), api.to_rgb8(mixed, 1))
