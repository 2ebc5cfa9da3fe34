"""GPU: rene-hip --direct PREFIX [--direct-frames N] on the Cornell .pbrt fixture -- the three files of a pass that covers the job's frames, equal
to the Python calls bit for bit, and the direct files alone (with the reason on an INFO line) where it does not."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from rene_amd import api, loader

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
PBRT = os.path.join(GOLDEN, "sample_scenes", "cornell-box", "scene.pbrt")
W, H = 100, 70


def _read_pfm(path):
    with open(path, "rb") as f:
        kind = f.readline().strip()
        w, h = map(int, f.readline().split())
        assert float(f.readline()) == -1.0
        ch = {b"PF": 3, b"Pf": 1}[kind]
        a = np.frombuffer(f.read(), "<f4").reshape(h, w, ch)
    return a[::-1]  # bottom row first in the file


def _loaded():
    loaded = loader.load_pbrt(PBRT)
    desc = loaded.desc  # the command line's override of the Film size: the projection's x axis rescaled to the new aspect, in fp32
    ratio = np.float32(np.float32(W) / np.float32(H)) / np.float32(np.float32(desc.xresolution) / np.float32(desc.yresolution))
    desc.uniform.projection_inv[0] = np.float32(np.float32(desc.uniform.projection_inv[0]) * ratio)
    desc.xresolution, desc.yresolution = W, H
    loaded.xres, loaded.yres = W, H
    return loaded


def test_the_command_line_writes_the_three_files(hip_lib, tmp_path):
    p = subprocess.run([CLI, PBRT, "--width", str(W), "--height", str(H), "--spp", "4", "--out", "o.png", "--direct", "d"], capture_output=True, text=True,
                       cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    assert sorted(os.listdir(tmp_path)) == ["d.direct.pfm", "d.direct.png", "d.indirect.pfm", "o.png"]
    assert "INFO direct-light pass over frames 0 .. 3" in p.stderr and "d.indirect.pfm (beauty - direct)" in p.stderr
    with api.Renderer(_loaded()) as r:
        r.render(0, 4)
        beauty = r.download(0)
        rec = r.direct(0, 4)  # the default of --direct-frames is the job's --spp
    direct, indirect = api.direct_mean(rec), api.indirect_mean(beauty, rec)
    assert _read_pfm(tmp_path / "d.direct.pfm").tobytes() == direct.tobytes()
    assert _read_pfm(tmp_path / "d.indirect.pfm").tobytes() == indirect.tobytes()
    assert (rec["hits"] > 0).mean() > 0.5 and direct.mean() > 0 and indirect.mean() > 0
    png = open(tmp_path / "d.direct.png", "rb").read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and png[16:26] == W.to_bytes(4, "big") + H.to_bytes(4, "big") + b"\x08\x02"  # 8-bit RGB
    import zlib
    at, idat = 8, b""
    while at < len(png):
        n, kind = int.from_bytes(png[at:at + 4], "big"), png[at + 4:at + 8]
        if kind == b"IDAT":
            idat += png[at + 8:at + 8 + n]
        at += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 3 * W)
    assert not rows[:, 0].any() and np.array_equal(rows[:, 1:].reshape(H, W, 3), api.to_rgb8(api.direct_sum(rec), 4))


def test_a_pass_over_other_frames_writes_the_direct_files_and_says_why(hip_lib, tmp_path):
    p = subprocess.run([CLI, PBRT, "--width", str(W), "--height", str(H), "--spp", "4", "--out", "o.png", "--direct", "d", "--direct-frames", "2"],
                       capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    assert sorted(os.listdir(tmp_path)) == ["d.direct.pfm", "d.direct.png", "o.png"]
    line = [l for l in p.stderr.splitlines() if l.startswith("INFO direct-light pass")]
    assert len(line) == 1 and "d.indirect.pfm is not written" in line[0] and "does not cover exactly the job's frames" in line[0]
    with api.Renderer(_loaded()) as r:
        rec = r.direct(0, 2)
    assert _read_pfm(tmp_path / "d.direct.pfm").tobytes() == api.direct_mean(rec).tobytes()
