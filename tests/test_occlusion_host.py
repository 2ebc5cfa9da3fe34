"""CPU: the host side of the occlusion pass (rene_occlusion, include/rene_hip.h) -- the header as C99, struct sizes against the ctypes mirrors,
defaults, the ABI version, every refusal that needs no GPU, and the command line's refusals and --help."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT
from rene_amd import abi, api, scenes

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
SYMBOLS = ("rene_occlusion_params_default", "rene_occlusion_bytes", "rene_occlusion", "rene_occlusion_buffer", "rene_download_occlusion",
           "rene_occlusion_samples")


def test_abi_structs_defaults_and_symbols(hip_lib):
    assert C.sizeof(abi.OcclusionPixel) == 32 == np.dtype(abi.OCCLUSION_DTYPE).itemsize
    assert C.sizeof(abi.OcclusionSample) == 48 == np.dtype(abi.OCCLUSION_SAMPLE_DTYPE).itemsize and C.sizeof(abi.OcclusionParams) == 24
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "rene_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %u %u\\n", '
            'sizeof(rene_occlusion_pixel), sizeof(rene_occlusion_sample), sizeof(rene_occlusion_params), offsetof(rene_occlusion_pixel, bent_sum), '
            'offsetof(rene_occlusion_sample, state), offsetof(rene_occlusion_sample, r1), offsetof(rene_occlusion_sample, r2), '
            'offsetof(rene_occlusion_params, radius), RENE_OCCLUSION_MAX_RAYS, RENE_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "s.c"), os.path.join(tmp, "s")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])  # (the header is C)
        assert subprocess.check_output([exe]).split() == [b"32", b"48", b"24", b"16", b"12", b"28", b"44", b"16", b"64", b"7"]
    assert abi.OcclusionPixel.bent_sum.offset == 16 and abi.OcclusionSample.r1.offset == 28 and abi.OcclusionSample.r2.offset == 44
    assert abi.OcclusionParams.radius.offset == 16 and abi.OCCLUSION_MAX_RAYS == 64 and abi.ABI_VERSION == 7 == hip_lib.rene_abi_version()
    for name in SYMBOLS:
        assert name in abi.EXPORTED_SYMBOLS and hasattr(hip_lib, name), name
    p = api.occlusion_params_default()
    assert (p.struct_size, p.first_frame, p.n_frames, p.rays, p.radius, p.flags) == (24, 0, 16, 1, 1.0, 0)
    assert api.occlusion_bytes(77, 45) == 77 * 45 * 32 and api.occlusion_bytes(16384, 16384) == 32 << 28 and api.occlusion_bytes(0, 9) == 0
    for m in ("occlusion", "occlusion_into", "occlusion_buffer", "occlusion_samples"):
        assert callable(getattr(api.Renderer, m))
    hip_lib.rene_occlusion_params_default(None)  # (a NULL destination: nothing happens)


BAD = (("struct_size", 20, "struct_size"), ("n_frames", 0, "n_frames"), ("n_frames", 65537, "n_frames"), ("rays", 0, "rays"), ("rays", 65, "rays"),
       ("radius", 0.001, "radius"), ("radius", 0.0, "radius"), ("radius", -1.0, "radius"), ("radius", 100001.0, "radius"),
       ("radius", float("inf"), "radius"), ("radius", float("nan"), "radius"), ("flags", 1, "flags"))


def test_parameters_are_checked_and_nothing_runs_without_a_gpu(hip_lib):
    L = hip_lib
    err = lambda: L.rene_last_error().decode()
    buf = np.zeros(96, np.uint8).ctypes.data_as(C.c_void_p)
    for field, value, word in BAD:
        p = api.occlusion_params_default()
        setattr(p, field, value)
        assert L.rene_occlusion(None, C.byref(p), None, 0) == -1 and word in err(), (field, value)
        assert L.rene_occlusion_samples(None, C.byref(p), buf, 2) == -1 and word in err(), (field, value)
    # the ends of the ranges are inside them
    for field, value in (("n_frames", 65536), ("rays", 64), ("radius", 100000.0), ("radius", 0.0011)):
        p = api.occlusion_params_default()
        setattr(p, field, value)
        assert L.rene_occlusion(None, C.byref(p), None, 0) == -1 and "NULL context" in err(), (field, value)
    # good parameters: what is missing is the context -- there is none without a GPU, and no CPU fallback
    assert L.rene_occlusion(None, None, None, 0) == -1 and "NULL context" in err()
    assert L.rene_occlusion_samples(None, None, buf, 2) == -1 and "NULL" in err()
    p, n = C.c_void_p(), C.c_size_t()
    assert L.rene_occlusion_buffer(None, C.byref(p), C.byref(n)) == -1 and "NULL" in err()
    assert L.rene_download_occlusion(None, buf, 96) == -1 and "NULL" in err()
    from conftest import has_gpu
    if not has_gpu():
        with pytest.raises(api.ReneError) as e:
            api.Renderer(scenes.cornell_box(16, 16)).occlusion()
        assert e.value.code == -3  # RENE_ERR_DEVICE


def test_the_command_line_refuses_before_it_loads_anything(hip_lib):
    def run(*args):
        return subprocess.run([CLI, "no-such.pbrt", *args], capture_output=True, text=True)
    r = run("--ao", "a", "--gpus", "2")
    assert r.returncode == 2 and "rene_occlusion" in r.stderr and "api.occlusion_merge" in r.stderr
    for bad in (("--ao-rays", "0"), ("--ao-rays", "65"), ("--ao-radius", "0"), ("--ao-radius", "1e6"), ("--ao-radius", "nan"), ("--ao-frames", "65537")):
        r = run("--ao", "a", *bad)
        assert r.returncode == 2 and "--ao-radius" in r.stderr and "--ao-rays" in r.stderr, bad
    assert run("--ao").returncode == 2 and run("--ao", "a", "--ao-rays").returncode == 2  # (a missing value)
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for word in ("--ao PREFIX", "--ao-radius R", "--ao-rays K", "--ao-frames N", "PREFIX.ao.pfm", "--gbuffer PREFIX", "--exr PATH"):
        assert word in r.stderr, word
