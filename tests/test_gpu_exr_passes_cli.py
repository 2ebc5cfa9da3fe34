"""GPU: `rene-hip --exr-passes` writes the file the Python call writes for the same job (rene_write_exr_passes against Renderer.exr_passes): the
passes the layers need run over the job's own frames, with the command line's occlusion rays and radius and its cap on the bounces."""
import os
import subprocess

import numpy as np
import pytest

import cryptomatte_reference as cr
import exr_passes_reference as pr
import exr_reference
from conftest import ROOT
from rene_amd import abi, api, loader
from test_cryptomatte_host import PBRT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
SPP = 8


def test_command_line(hip_lib, tmp_path):
    p = tmp_path / "scene.pbrt"
    p.write_text(PBRT)
    names = ["sky", None, "lamp 1"]
    run = subprocess.run([CLI, str(p), "--spp", str(SPP), "--exr-passes", "all.exr", "--exr-compression", "zips", "--exr-light-names", "sky,,lamp 1", "--ao-rays", "2",
                          "--ao-radius", "0.5", "--bounces-max-depth", "6"], capture_output=True, text=True, cwd=tmp_path)
    assert run.returncode == 0, run.stderr
    info = [l for l in run.stderr.splitlines() if l.startswith("INFO pass layers")]
    assert len(info) == 1 and "frames 0 .. 7" in info[0] and "layers 0x7f" in info[0] and "130 bytes per pixel" in info[0]
    got = (tmp_path / "all.exr").read_bytes()
    assert not (tmp_path / "all.exr.tmp").exists()
    with api.Renderer(loader.load_pbrt(str(p))) as r:
        r.render(0, SPP)
        r.occlusion(0, SPP, 2, 0.5), r.direct(0, SPP), r.bounces(0, SPP, 6), r.lights(0, SPP)
        assert r.exr_passes(group_names=names, compression="zips") == got  # the Python route writes the same file
        plain = r.exr_passes(group_names=names)
        w, h = r.xres, r.yres
    attrs = {n: v for n, _, v in cr.walk_header(got)[0]}
    assert attrs["compression"] == b"\x02" and attrs["rene/lightGroups"] == b'{"light0":"sky","light2":"lamp 1"}'
    # the layers of the options the command line already has, uncompressed, beside their .pfm files
    run = subprocess.run([CLI, str(p), "--spp", str(SPP), "--exr-passes", "two.exr", "--ao", "a", "--ao-frames", "4", "--lights", "l"], capture_output=True, text=True, cwd=tmp_path)
    assert run.returncode == 0, run.stderr
    pw, ph, chans = exr_reference.parse((tmp_path / "two.exr").read_bytes())
    assert (pw, ph) == (w, h) and list(chans) == pr.channel_names(abi.EXRP_AO | abi.EXRP_BENT | abi.EXRP_LIGHTS)
    assert (tmp_path / "a.ao.pfm").exists() and (tmp_path / "l.group0.pfm").exists() and (tmp_path / "l.groups.txt").exists()  # (as before)
    whole = exr_reference.parse(plain)[2]
    assert chans["light1.G"].tobytes() == whole["light1.G"].tobytes()  # the same frames, the same grouping
    with api.Renderer(loader.load_pbrt(str(p))) as r:
        r.occlusion(0, SPP)  # (the job's frames and the default ray and radius, not --ao-frames 4)
        ao = exr_reference.parse(r.exr_passes(layers="ao"))[2]["ao"]
    assert chans["ao"].tobytes() == ao.tobytes()
    one = subprocess.run([CLI, str(p), "--spp", str(SPP), "--exr-passes", "one.exr", "--exr-pass-layers", "indirect,length"], capture_output=True, text=True, cwd=tmp_path)
    assert one.returncode == 0, one.stderr
    chans = exr_reference.parse((tmp_path / "one.exr").read_bytes())[2]
    assert list(chans) == ["indirect.B", "indirect.G", "indirect.R", "pathlength"] and chans["indirect.R"].tobytes() == whole["indirect.R"].tobytes()
    assert chans["pathlength"].astype(np.float32).max() > 1
    for bad in (["--gpus", "2"], ["--exr-pass-layers", "beauty"], ["--adaptive", "--target-noise", "0.5"]):
        assert subprocess.run([CLI, str(p), "--spp", str(SPP), "--exr-passes", "bad.exr"] + bad, capture_output=True, cwd=tmp_path).returncode == 2
