"""CPU: the host side of the direct-light pass (rene_direct, include/rene_hip.h) -- the header as C99, struct sizes against the ctypes mirrors,
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
SYMBOLS = ("rene_direct_params_default", "rene_direct_bytes", "rene_direct", "rene_direct_buffer", "rene_download_direct", "rene_direct_samples")


def test_abi_structs_defaults_and_symbols(hip_lib):
    assert C.sizeof(abi.DirectPixel) == 48 == np.dtype(abi.DIRECT_DTYPE).itemsize
    assert C.sizeof(abi.DirectSample) == 64 == np.dtype(abi.DIRECT_SAMPLE_DTYPE).itemsize and C.sizeof(abi.DirectParams) == 16
    fields = ("sizeof(rene_direct_pixel)", "sizeof(rene_direct_sample)", "sizeof(rene_direct_params)", "offsetof(rene_direct_pixel, hits)",
              "offsetof(rene_direct_pixel, distant)", "offsetof(rene_direct_pixel, n)", "offsetof(rene_direct_pixel, sampled)",
              "offsetof(rene_direct_sample, state)", "offsetof(rene_direct_sample, pdf)", "offsetof(rene_direct_sample, wi)",
              "offsetof(rene_direct_sample, second)", "offsetof(rene_direct_sample, sampled)", "offsetof(rene_direct_params, flags)",
              "(size_t)RENE_DIRECT_MAX_FRAMES", "(size_t)RENE_DIRECT_MISS", "(size_t)RENE_DIRECT_LIGHT", "(size_t)RENE_DIRECT_BSDF", "(size_t)RENE_DIRECT_PLAIN",
              "(size_t)RENE_DIRECT_ENDED_PDF", "(size_t)RENE_DIRECT_ENDED_ZERO", "(size_t)RENE_DIRECT_SECOND_NONE", "(size_t)RENE_DIRECT_SECOND_MISS",
              "(size_t)RENE_DIRECT_SECOND_SURFACE", "(size_t)RENE_DIRECT_SECOND_EMITTER", "(size_t)RENE_ABI_VERSION")
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "rene_hip.h"\nint main(void){size_t v[] = {' + ", ".join(fields) +
            '};for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%zu ", v[i]);return 0;}\n')
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "s.c"), os.path.join(tmp, "s")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])  # (the header is C)
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [48, 64, 16, 12, 16, 28, 32, 12, 28, 32, 44, 48, 12, 65536, 0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 7]
    P, S = abi.DirectPixel, abi.DirectSample
    assert (P.hits.offset, P.distant.offset, P.n.offset, P.sampled.offset, P.reserved.offset) == (12, 16, 28, 32, 44)
    assert (S.state.offset, S.distant.offset, S.pdf.offset, S.wi.offset, S.second.offset, S.sampled.offset, S.reserved.offset) == (12, 16, 28, 32, 44, 48, 60)
    for dtype, struct in ((abi.DIRECT_DTYPE, P), (abi.DIRECT_SAMPLE_DTYPE, S)):
        d = np.dtype(dtype)
        assert {k: d.fields[k][1] for k in d.names} == {k: getattr(struct, k).offset for k, _ in struct._fields_}
    assert (abi.DIRECT_MISS, abi.DIRECT_LIGHT, abi.DIRECT_BSDF, abi.DIRECT_PLAIN, abi.DIRECT_ENDED_PDF, abi.DIRECT_ENDED_ZERO) == (0, 1, 2, 3, 4, 5)
    assert (abi.DIRECT_SECOND_NONE, abi.DIRECT_SECOND_MISS, abi.DIRECT_SECOND_SURFACE, abi.DIRECT_SECOND_EMITTER) == (0, 1, 2, 3)
    assert abi.DIRECT_MAX_FRAMES == 65536 and abi.ABI_VERSION == 7 == hip_lib.rene_abi_version()  # added symbols: no version change
    for name in SYMBOLS:
        assert name in abi.EXPORTED_SYMBOLS and hasattr(hip_lib, name), name
    p = api.direct_params_default()
    assert (p.struct_size, p.first_frame, p.n_frames, p.flags) == (16, 0, 16, 0)
    assert api.direct_bytes(48, 40) == 48 * 40 * 48 and api.direct_bytes(16384, 16384) == 48 << 28 and api.direct_bytes(0, 9) == 0
    for m in ("direct", "direct_into", "direct_buffer", "direct_samples"):
        assert callable(getattr(api.Renderer, m))
    for f in ("direct_sum", "direct_mean", "direct_merge", "indirect_mean"):
        assert callable(getattr(api, f))
    hip_lib.rene_direct_params_default(None)  # (a NULL destination: nothing happens)


BAD = (("struct_size", 12, "struct_size"), ("struct_size", 0, "struct_size"), ("n_frames", 0, "n_frames"), ("n_frames", 65537, "n_frames"),
       ("flags", 1, "flags"), ("flags", 1 << 31, "flags"))


def test_parameters_are_checked_and_nothing_runs_without_a_gpu(hip_lib):
    L = hip_lib
    err = lambda: L.rene_last_error().decode()
    buf = np.zeros(128, np.uint8).ctypes.data_as(C.c_void_p)
    for field, value, word in BAD:
        p = api.direct_params_default()
        setattr(p, field, value)
        assert L.rene_direct(None, C.byref(p), None, 0) == -1 and word in err(), (field, value)
        assert L.rene_direct_samples(None, C.byref(p), buf, 2) == -1 and word in err(), (field, value)
    # the ends of the range are inside it
    for value in (1, 65536):
        p = api.direct_params_default()
        p.n_frames = value
        assert L.rene_direct(None, C.byref(p), None, 0) == -1 and "NULL context" in err(), value
    # good parameters: what is missing is the context -- there is none without a GPU, and no CPU fallback
    assert L.rene_direct(None, None, None, 0) == -1 and "NULL context" in err()
    assert L.rene_direct_samples(None, None, buf, 2) == -1 and "NULL" in err()
    p, n = C.c_void_p(), C.c_size_t()
    assert L.rene_direct_buffer(None, C.byref(p), C.byref(n)) == -1 and "NULL" in err()
    assert L.rene_download_direct(None, buf, 96) == -1 and "NULL" in err()
    from conftest import has_gpu
    if not has_gpu():
        with pytest.raises(api.ReneError) as e:
            api.Renderer(scenes.cornell_box(16, 16)).direct()
        assert e.value.code == -3  # RENE_ERR_DEVICE


def test_the_command_line_refuses_before_it_loads_anything(hip_lib):
    def run(*args):
        return subprocess.run([CLI, "no-such.pbrt", *args], capture_output=True, text=True)
    r = run("--direct", "d", "--gpus", "2")
    assert r.returncode == 2 and "rene_direct" in r.stderr and "api.direct_merge" in r.stderr
    r = run("--direct", "d", "--direct-frames", "65537")
    assert r.returncode == 2 and "--direct-frames" in r.stderr
    assert run("--direct").returncode == 2 and run("--direct", "d", "--direct-frames").returncode == 2  # (a missing value)
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for word in ("--direct PREFIX", "--direct-frames N", "PREFIX.direct.pfm", "PREFIX.indirect.pfm", "--ao PREFIX", "--gbuffer PREFIX"):
        assert word in r.stderr, word
