"""CPU: the host side of the output transform on the device (rene_output_8bit, include/rene_hip.h).  The device's sRGB bytes are a lookup in
rene_output_thresholds' table, so what is checked here, without a GPU, is the argument that makes the lookup exact: the table is derived from
rene_to_rgb8 itself, it is strictly increasing, T[k] is the smallest float mapped to k + 1, and counting the thresholds <= v reproduces
rene_to_rgb8 -- on random floats, around every threshold, on the specials, and (selftest/output_table_check) on every non-negative finite float."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
from rene_amd import abi, api

CSRC = os.path.join(ROOT, "rene_amd", "csrc")
SPECIALS = np.array([0.0, -0.0, -1.0, -1e-30, -1e30, 1e-45, -1e-45, 1e-39, 1.1754942e-38, np.nan, -np.nan, np.inf, -np.inf, 1e30, 0.0031308,
                     np.nextafter(np.float32(0.0031308), np.float32(1)), 1.0, np.nextafter(np.float32(1), np.float32(0)), 1.5, 3.4e38], np.float32)


def around(t, ulps=2):
    """Every value of t and its `ulps` neighbours on either side."""
    out = [t]
    lo = hi = t
    for _ in range(ulps):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return np.concatenate(out).astype(np.float32)


def test_thresholds_are_the_steps_of_to_rgb8(hip_lib):
    T = api.output_thresholds()
    assert T.dtype == np.float32 and T.shape == (255,)
    assert (T > 0).all() and (np.diff(T) > 0).all() and T[-1] <= 1.0
    k = np.arange(255)
    assert np.array_equal(api.to_rgb8(T, 1), k + 1)
    assert np.array_equal(api.to_rgb8(np.nextafter(T, np.float32(0)), 1), k)


def test_counting_thresholds_is_to_rgb8(hip_lib):
    T = api.output_thresholds()
    rng = np.random.default_rng(20)
    v = np.concatenate([(rng.random(1 << 20) * 1.5).astype(np.float32), around(T), SPECIALS])
    with np.errstate(invalid="ignore"):
        count = np.searchsorted(T, np.where(np.isnan(v), np.float32(-1), v), "right")  # (a NaN counts no threshold: `v >= T[k]` is false)
    assert np.array_equal(count, api.to_rgb8(v, 1))
    sp = api.to_rgb8(SPECIALS, 1)
    assert sp[np.isnan(SPECIALS)].max() == 0 and sp[SPECIALS <= 0].max() == 0 and sp[SPECIALS == np.inf].min() == 255 and sp[SPECIALS == 1e30].min() == 255


def test_every_float_through_the_selftest(hip_lib):
    exe = os.path.join(CSRC, "selftest", "output_table_check")
    if not os.path.exists(exe):
        api.build()
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok: 2139095040 floats, 255 steps"), p.stdout + p.stderr


def test_params_and_refusals_without_a_gpu(hip_lib):
    p = api.output_params_default()
    assert (p.struct_size, p.source, p.format, p.reserved) == (C.sizeof(abi.OutputParams), abi.OUTPUT_RADIANCE, abi.OUTPUT_RGB8, 0) and p.struct_size == 16
    assert [abi.OUTPUT_RADIANCE, abi.OUTPUT_NORMAL, abi.OUTPUT_ALBEDO, abi.OUTPUT_DENOISED, abi.OUTPUT_DENOISED_MEAN, abi.OUTPUT_ROBUST] == list(range(6))
    header = open(os.path.join(ROOT, "include", "rene_hip.h")).read()
    for name in ("RADIANCE", "NORMAL", "ALBEDO", "DENOISED", "DENOISED_MEAN", "ROBUST", "RGB8", "RGBA8", "SRGB", "AOV", "AOV_NORMAL"):
        assert int(re.search(rf"RENE_OUTPUT_{name} = (\d+)", header).group(1)) == getattr(abi, "OUTPUT_" + name), name
    L = hip_lib
    assert L.rene_output_8bit(None, C.byref(p), None, 0) == -1 and b"NULL context" in L.rene_last_error()
    ptr, n = C.c_void_p(), C.c_size_t()
    assert L.rene_output_buffer(None, C.byref(ptr), C.byref(n)) == -1
    assert L.rene_download_output(None, None, 0) == -1
    one = np.zeros(1, np.float32)
    out = np.zeros(1, np.uint8)
    assert L.rene_output_probe(0, 3, 1, one.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == -1 and b"transform" in L.rene_last_error()
    assert L.rene_output_probe(0, 0, 1, None, out.ctypes.data_as(C.c_void_p)) == -1
    assert L.rene_output_probe(0, 0, 0, None, None) == 0  # nothing to do, no device touched
    try:
        api.output_probe(one, "gamma")
    except ValueError:
        pass
    else:
        raise AssertionError("output_probe accepted an unknown transform")
    L.rene_output_params_default(None)  # tolerated
    L.rene_output_thresholds(None)


def test_the_unit_is_built_with_the_robust_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    assert "kernels_output.o" in objs
    rule = re.search(r"^kernels_output\.o: kernels_output\.hip \$\(HDRS\)\n\t(.*)$", mk, re.M).group(1)
    assert "$(ROBUSTFLAGS)" in rule and "$(HIPFLAGS)" not in rule and "$(RESFLAGS)" in rule and "2> kernels_output.res" in rule
    variant = mk[mk.index("\nvariant:"):mk.index("\nclean:")]
    assert re.search(r"\$\(ROBUSTFLAGS\) \$\(RESFLAGS\) \$\(EXTRA\) -c -o var_\$\(NAME\)/kernels_output\.o kernels_output\.hip", variant)
    assert "selftest/output_table_check" in re.search(r"^all: (.*)$", mk, re.M).group(1).split()
