"""CPU: the host side of the bounce pass (rene_bounces, include/rene_hip.h) -- the header as C99, struct sizes and offsets against the ctypes
mirrors, defaults, the ABI version, every refusal that needs no GPU, and the command line's refusals and --help."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT
from rene_amd import abi, api, scenes

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
SYMBOLS = ("rene_bounces_params_default", "rene_bounces_bytes", "rene_bounces", "rene_bounces_buffer", "rene_download_bounces", "rene_bounces_samples")


def test_abi_structs_defaults_and_symbols(hip_lib):
    assert C.sizeof(abi.BouncesPixel) == 176 == np.dtype(abi.BOUNCES_DTYPE).itemsize
    assert C.sizeof(abi.BouncesSample) == 176 == np.dtype(abi.BOUNCES_SAMPLE_DTYPE).itemsize
    assert C.sizeof(abi.BouncesParams) == 20 and C.sizeof(abi.BouncesBucket) == 16 == np.dtype(abi.BOUNCES_BUCKET_DTYPE).itemsize
    fields = ("sizeof(rene_bounces_params)", "sizeof(rene_bounces_pixel)", "sizeof(rene_bounces_sample)", "sizeof(rene_bounces_bucket)",
              "offsetof(rene_bounces_params, max_depth)", "offsetof(rene_bounces_params, flags)", "offsetof(rene_bounces_bucket, reached)",
              "offsetof(rene_bounces_pixel, bucket[9])", "offsetof(rene_bounces_pixel, n)", "offsetof(rene_bounces_pixel, length_sum)",
              "offsetof(rene_bounces_pixel, length_max)", "offsetof(rene_bounces_pixel, capped)", "offsetof(rene_bounces_sample, n)",
              "offsetof(rene_bounces_sample, length)", "offsetof(rene_bounces_sample, end)", "offsetof(rene_bounces_sample, reserved)",
              "(size_t)RENE_BOUNCES_MAX_FRAMES", "(size_t)RENE_BOUNCES_BUCKETS", "(size_t)RENE_BOUNCES_MAX_DEPTH", "(size_t)RENE_BOUNCES_END_MISS",
              "(size_t)RENE_BOUNCES_END_PDF", "(size_t)RENE_BOUNCES_END_ZERO", "(size_t)RENE_BOUNCES_END_ROULETTE", "(size_t)RENE_BOUNCES_END_CAP",
              "(size_t)RENE_ABI_VERSION")
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "rene_hip.h"\nint main(void){size_t v[] = {' + ", ".join(fields) +
            '};for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%zu ", v[i]);return 0;}\n')
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "s.c"), os.path.join(tmp, "s")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])  # (the header is C)
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [20, 176, 176, 16, 12, 16, 12, 144, 160, 164, 168, 172, 160, 164, 168, 172, 65536, 10, 50, 0, 1, 2, 3, 4, 7]
    P, S = abi.BouncesPixel, abi.BouncesSample
    assert (P.bucket.offset, P.n.offset, P.length_sum.offset, P.length_max.offset, P.capped.offset) == (0, 160, 164, 168, 172)
    assert (S.bucket.offset, S.n.offset, S.length.offset, S.end.offset, S.reserved.offset) == (0, 160, 164, 168, 172)
    assert (abi.BouncesBucket.sum.offset, abi.BouncesBucket.reached.offset) == (0, 12)
    for dtype, struct in ((abi.BOUNCES_DTYPE, P), (abi.BOUNCES_SAMPLE_DTYPE, S), (abi.BOUNCES_BUCKET_DTYPE, abi.BouncesBucket)):
        d = np.dtype(dtype)
        assert {k: d.fields[k][1] for k in d.names} == {k: getattr(struct, k).offset for k, _ in struct._fields_}
    assert np.dtype(abi.BOUNCES_DTYPE).fields["bucket"][0].shape == (10,)
    assert (abi.BOUNCES_END_MISS, abi.BOUNCES_END_PDF, abi.BOUNCES_END_ZERO, abi.BOUNCES_END_ROULETTE, abi.BOUNCES_END_CAP) == (0, 1, 2, 3, 4)
    assert (abi.BOUNCES_MAX_FRAMES, abi.BOUNCES_BUCKETS, abi.BOUNCES_MAX_DEPTH) == (65536, 10, 50)
    assert abi.ABI_VERSION == 7 == hip_lib.rene_abi_version()  # added symbols: no version change
    for name in SYMBOLS:
        assert name in abi.EXPORTED_SYMBOLS and hasattr(hip_lib, name), name
    p = api.bounces_params_default()
    assert (p.struct_size, p.first_frame, p.n_frames, p.max_depth, p.flags) == (20, 0, 16, 0, 0)
    assert api.bounces_bytes(48, 40) == 48 * 40 * 176 and api.bounces_bytes(16384, 16384) == 176 << 28 and api.bounces_bytes(0, 9) == 0
    for m in ("bounces", "bounces_into", "bounces_buffer", "bounces_samples"):
        assert callable(getattr(api.Renderer, m))
    for f in ("bounces_sum", "bounces_depth_mean", "bounces_mean_length", "bounces_reached", "bounces_merge"):
        assert callable(getattr(api, f))
    hip_lib.rene_bounces_params_default(None)  # (a NULL destination: nothing happens)


BAD = (("struct_size", 16, "struct_size"), ("struct_size", 0, "struct_size"), ("n_frames", 0, "n_frames"), ("n_frames", 65537, "n_frames"),
       ("max_depth", 51, "max_depth"), ("max_depth", 1 << 31, "max_depth"), ("flags", 1, "flags"), ("flags", 1 << 31, "flags"))


def test_parameters_are_checked_and_nothing_runs_without_a_gpu(hip_lib):
    L = hip_lib
    err = lambda: L.rene_last_error().decode()
    buf = np.zeros(512, np.uint8).ctypes.data_as(C.c_void_p)
    for field, value, word in BAD:
        p = api.bounces_params_default()
        setattr(p, field, value)
        assert L.rene_bounces(None, C.byref(p), None, 0) == -1 and word in err() and "rene_bounces" in err(), (field, value)
        assert L.rene_bounces_samples(None, C.byref(p), buf, 2) == -1 and word in err() and "rene_bounces" in err(), (field, value)
    # the ends of the ranges are inside them
    for field, value in (("n_frames", 1), ("n_frames", 65536), ("max_depth", 0), ("max_depth", 1), ("max_depth", 50)):
        p = api.bounces_params_default()
        setattr(p, field, value)
        assert L.rene_bounces(None, C.byref(p), None, 0) == -1 and "rene_bounces: NULL context" in err(), (field, value)
    # good parameters: what is missing is the context -- there is none without a GPU, and no CPU fallback
    assert L.rene_bounces(None, None, None, 0) == -1 and err() == "rene_bounces: NULL context"
    assert L.rene_bounces_samples(None, None, buf, 2) == -1 and "rene_bounces_samples: NULL" in err()
    p, n = C.c_void_p(), C.c_size_t()
    assert L.rene_bounces_buffer(None, C.byref(p), C.byref(n)) == -1 and "rene_bounces_buffer" in err() and "NULL" in err()
    assert L.rene_download_bounces(None, buf, 352) == -1 and "rene_download_bounces" in err() and "NULL" in err()
    from conftest import has_gpu
    if not has_gpu():
        with pytest.raises(api.ReneError) as e:
            api.Renderer(scenes.cornell_box(16, 16)).bounces()
        assert e.value.code == -3  # RENE_ERR_DEVICE


def test_the_command_line_refuses_before_it_loads_anything(hip_lib):
    def run(*args):
        return subprocess.run([CLI, "no-such.pbrt", *args], capture_output=True, text=True)
    r = run("--bounces", "b", "--gpus", "2")
    assert r.returncode == 2 and "rene_bounces" in r.stderr and "api.bounces_merge" in r.stderr
    r = run("--bounces", "b", "--bounces-frames", "65537")
    assert r.returncode == 2 and "--bounces-frames" in r.stderr
    r = run("--bounces", "b", "--bounces-max-depth", "51")
    assert r.returncode == 2 and "--bounces-max-depth" in r.stderr
    assert run("--bounces").returncode == 2 and run("--bounces", "b", "--bounces-frames").returncode == 2  # (a missing value)
    assert run("--bounces", "b", "--bounces-max-depth").returncode == 2
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for word in ("--bounces PREFIX", "--bounces-frames N", "--bounces-max-depth D", "PREFIX.depth0.pfm", "PREFIX.length.pfm", "PREFIX.length.png", "--direct PREFIX"):
        assert word in r.stderr, word
