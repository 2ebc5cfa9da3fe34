"""GPU: rene-hip --bounces PREFIX [--bounces-frames N] [--bounces-max-depth D] on the Cornell .pbrt fixture -- the ten depth files, the length map
and its grey image, equal to the Python calls bit for bit; under a cap the files from the cap on are black."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT
from rene_amd import api
from test_gpu_direct_cli import H, PBRT, W, _loaded, _read_pfm

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
FILES = sorted([f"b.depth{d}.pfm" for d in range(10)] + ["b.length.pfm", "b.length.png", "o.png"])


def _grey_png(path):
    png = open(path, "rb").read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and png[16:26] == W.to_bytes(4, "big") + H.to_bytes(4, "big") + b"\x08\x00"  # 8-bit grey
    at, idat = 8, b""
    while at < len(png):
        n, kind = int.from_bytes(png[at:at + 4], "big"), png[at + 4:at + 8]
        if kind == b"IDAT":
            idat += png[at + 8:at + 8 + n]
        at += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + W)
    assert not rows[:, 0].any()
    return rows[:, 1:]


def test_the_command_line_writes_the_depth_files_and_the_length_map(hip_lib, tmp_path):
    p = subprocess.run([CLI, PBRT, "--width", str(W), "--height", str(H), "--spp", "4", "--out", "o.png", "--bounces", "b"], capture_output=True, text=True,
                       cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    assert sorted(os.listdir(tmp_path)) == FILES
    assert "INFO bounce pass over frames 0 .. 3, at most 50 iterations per path" in p.stderr
    with api.Renderer(_loaded()) as r:
        rec = r.bounces(0, 4)  # the default of --bounces-frames is the job's --spp
    for d in range(10):
        assert _read_pfm(tmp_path / f"b.depth{d}.pfm").tobytes() == api.bounces_depth_mean(rec, d).tobytes(), d
    length = api.bounces_mean_length(rec)
    assert _read_pfm(tmp_path / "b.length.pfm")[..., 0].tobytes() == length.tobytes()
    assert api.bounces_depth_mean(rec, 0).sum() > 0 and api.bounces_depth_mean(rec, 1).sum() > 0 and length.min() >= 1
    grey = np.floor(np.float32(255) * (length / length.max()) + np.float32(0.5)).astype(np.uint8)
    assert np.array_equal(_grey_png(tmp_path / "b.length.png"), grey) and grey.max() == 255


def test_a_cap_of_two_leaves_the_deeper_files_black(hip_lib, tmp_path):
    p = subprocess.run([CLI, PBRT, "--width", str(W), "--height", str(H), "--spp", "4", "--out", "o.png", "--bounces", "b", "--bounces-frames", "2",
                        "--bounces-max-depth", "2"], capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    assert sorted(os.listdir(tmp_path)) == FILES
    assert "INFO bounce pass over frames 0 .. 1, at most 2 iterations per path" in p.stderr
    with api.Renderer(_loaded()) as r:
        rec, free = r.bounces(0, 2, max_depth=2), r.bounces(0, 2)
    assert rec["length_max"].max() == 2 and rec["capped"].sum() > 0
    for d in range(10):
        got = _read_pfm(tmp_path / f"b.depth{d}.pfm")
        assert got.tobytes() == api.bounces_depth_mean(rec, d).tobytes(), d
        if d >= 2:
            assert not got.any(), d  # black from the cap on
        else:
            assert got.tobytes() == api.bounces_depth_mean(free, d).tobytes() and got.sum() > 0, d  # and the job's own below it
    assert _read_pfm(tmp_path / "b.length.pfm")[..., 0].tobytes() == api.bounces_mean_length(rec).tobytes()
