"""CPU: the host side of the tone-mapped output transform and of the luminance histogram (include/rene_hip.h: rene_output_tonemapped,
rene_luminance_histogram).  The header specifies both operation by operation and tests/tonemap_reference.py restates them in numpy; here the
library's host functions -- the same arithmetic as the device code, which tests/test_gpu_tonemap.py compares with them -- are held against that
restatement with array_equal on bytes and integers, without a GPU."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import tonemap_reference as tr
from conftest import ROOT
from rene_amd import abi, api

CSRC = os.path.join(ROOT, "rene_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "rene_hip.h")
F = np.float32
NEW_SYMBOLS = ["rene_tonemap_params_default", "rene_output_tonemapped", "rene_luminance_histogram", "rene_luminance_combine",
               "rene_luminance_mean_bin_x256", "rene_luminance_percentile_bin", "rene_auto_exposure_e8", "rene_exposure_scale", "rene_tonemap_rgb8",
               "rene_luminance_histogram_host", "rene_tonemap_probe"]


def stats_of(counts, n_dark=0):
    s = abi.LuminanceStats()
    s.struct_size = C.sizeof(s)
    for b, c in enumerate(counts):
        s.counts[b] = int(c)
    s.n_dark = n_dark
    s.n_pixels = int(sum(int(c) for c in counts)) + n_dark
    return s


def test_header_is_c99_and_the_abi_is_the_one_it_was(hip_lib):
    prog = ('#include <stdio.h>\n#include "rene_hip.h"\nstatic const float M[8] = RENE_EXPOSURE_MANTISSAS;\nint main(void){\n'
            'printf("%zu %zu %zu %d %d %d %d %d\\n", sizeof(rene_output_params), sizeof(rene_tonemap_params), sizeof(rene_luminance_stats), RENE_ABI_VERSION,\n'
            '       RENE_TONEMAP_CLAMP, RENE_TONEMAP_REINHARD, RENE_TONEMAP_ACES, RENE_EXPOSURE_KEY_E8);\n'
            'for (int k = 0; k < 8; ++k) printf("%a\\n", (double)M[k]);\nreturn 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), src, "-o", exe])
        lines = subprocess.check_output([exe]).decode().splitlines()
    assert lines[0].split() == ["16", str(C.sizeof(abi.TonemapParams)), str(C.sizeof(abi.LuminanceStats)), "7", "0", "1", "2", "-20"]
    assert C.sizeof(abi.OutputParams) == 16 and C.sizeof(abi.TonemapParams) == 32 and C.sizeof(abi.LuminanceStats) == 4 * 259
    assert hip_lib.rene_abi_version() == abi.ABI_VERSION == 7  # added symbols: no version change
    # the eight literals are (float)2^(k / 8), and so are the restatement's
    assert [float.fromhex(l) for l in lines[1:9]] == [float(F(2 ** (k / 8))) for k in range(8)] == [float(m) for m in tr.M]
    text = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert name in abi.EXPORTED_SYMBOLS and hasattr(hip_lib, name) and re.search(r"\b" + name + r"\(", text), name
    assert (abi.TONEMAP_CLAMP, abi.TONEMAP_REINHARD, abi.TONEMAP_ACES) == (tr.CLAMP, tr.REINHARD, tr.ACES) == (0, 1, 2)
    assert (abi.EXPOSURE_KEY_E8, abi.EXPOSURE_E8_MIN, abi.EXPOSURE_E8_MAX) == (-20, tr.E8_MIN, tr.E8_MAX)
    for name in ("KEY_E8", "E8_MIN", "E8_MAX"):
        assert int(re.search(rf"#define RENE_EXPOSURE_{name} \(?(-?\d+)", text).group(1)) == getattr(abi, "EXPOSURE_" + name)
    p = api.tonemap_params_default()
    assert (p.struct_size, p.source, p.format, p.op, p.scale, p.white, list(p.reserved)) == (32, abi.OUTPUT_RADIANCE, abi.OUTPUT_RGB8, abi.TONEMAP_CLAMP, 1.0, 4.0, [0, 0])


@pytest.fixture(scope="module")
def values(hip_lib):
    T = api.output_thresholds()
    return T, tr.value_set(T)


@pytest.mark.parametrize("op", list(tr.OPS))
def test_tonemap_rgb8_equals_the_restatement(values, op):
    T, v = values
    for scale in tr.SCALES:
        for white in (4.0, 1.5):
            if op != "reinhard" and white != 4.0:
                continue
            got = api.tonemap_rgb8(v, op, scale, white)
            want = tr.tonemap_rgb8(v, tr.OPS[op], scale, white, T)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (op, float(scale), white, len(bad), [(v[i].tolist(), int(got[i, c]), int(want[i, c])) for i, c in bad[:4]])
            assert len(np.unique(got)) == 256  # every byte is met
    four = np.concatenate([v[:4096], np.full((4096, 1), 7.0, np.float32)], -1)  # a fourth channel is skipped
    assert np.array_equal(api.tonemap_rgb8(four, op, 2.0), api.tonemap_rgb8(v[:4096], op, 2.0))


def test_the_properties_the_header_promises(values):
    T, v = values
    assert np.array_equal(api.tonemap_rgb8(v, "clamp", 1.0), api.to_rgb8(v, 1))  # CLAMP at scale 1 is rene_to_rgb8
    for op in tr.OPS:
        for scale in tr.SCALES + [F(1e-30), F(1e30)]:
            got = api.tonemap_rgb8(v, op, scale)
            with np.errstate(invalid="ignore"):
                assert (got[np.isposinf(v)] == 255).all(), (op, scale)  # a +inf mean: 255
                assert (got[np.isnan(v) | (v < 0)] == 0).all(), (op, scale)  # NaN and negative means: 0
            assert not api.tonemap_rgb8(np.zeros((5, 3), np.float32), op, scale).any()  # (N_t == 0: the mean is 0)


def test_refusals_of_the_host_functions(hip_lib):
    L = hip_lib
    v = np.ones((2, 3), np.float32)
    out = np.zeros((2, 3), np.uint8)
    call = lambda ch, op, scale, white: L.rene_tonemap_rgb8(v.ctypes.data_as(C.c_void_p), 2, ch, op, scale, white, out.ctypes.data_as(C.c_void_p))
    assert call(3, 0, 1.0, 4.0) == 0
    assert call(3, 3, 1.0, 4.0) == -1 and b"op" in L.rene_last_error()
    assert call(2, 0, 1.0, 4.0) == -1 and b"channels" in L.rene_last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(3, 0, bad, 4.0) == -1 and b"scale" in L.rene_last_error()
        assert call(3, 1, 1.0, bad) == -1 and b"white" in L.rene_last_error()
    assert L.rene_tonemap_rgb8(None, 2, 3, 0, 1.0, 4.0, out.ctypes.data_as(C.c_void_p)) == -1
    st = abi.LuminanceStats()
    assert L.rene_luminance_histogram_host(None, 2, 3, C.byref(st)) == -1 and L.rene_luminance_histogram_host(v.ctypes.data_as(C.c_void_p), 2, 5, C.byref(st)) == -1
    p = api.tonemap_params_default()
    assert L.rene_output_tonemapped(None, C.byref(p), None, 0) == -1 and b"NULL context" in L.rene_last_error()
    assert L.rene_luminance_histogram(None, 0, C.byref(st)) == -1
    assert L.rene_tonemap_probe(0, 3, 1.0, 4.0, 1, v.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == -1 and b"op" in L.rene_last_error()
    assert L.rene_tonemap_probe(0, 0, 0.0, 4.0, 1, v.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == -1
    assert L.rene_tonemap_probe(0, 0, 1.0, 4.0, 0, None, None) == 0  # nothing to do, no device touched
    L.rene_tonemap_params_default(None)  # tolerated
    for fn in (api.tonemap_rgb8, api.tonemap_probe):
        with pytest.raises(ValueError):
            fn(v, "filmic")


def test_histogram_on_and_beside_every_bin_edge(hip_lib):
    edges = tr.bin_edges()
    assert edges.size == 257 and edges[0] == F(2.0 ** -20) and edges[-1] == 4096.0
    l = np.concatenate([tr.SPECIALS, [F(1e-38), F(2.0 ** -21), F(5000.0)]]).astype(np.float32)  # grey pixels: the dark values and the clamped ends
    assert np.array_equal(tr.luminance_bins(edges[:-1]), np.arange(256)) and tr.luminance_bins(edges[-1:])[0] == 255
    assert np.array_equal(tr.luminance_bins(np.nextafter(edges[1:], F(0))), np.arange(256))
    assert (tr.luminance_bins(np.array([0.0, -0.0, -1.0, np.nan, -np.inf], np.float32)) == -1).all()
    assert tr.luminance_bins(np.array([1e-45, 1e-39, 2.0 ** -21, np.inf, 3.4e38], np.float32)).tolist() == [0, 0, 0, 255, 255]
    means = np.concatenate([tr.edge_pixels(), np.stack([l, l, l], -1)])
    with np.errstate(all="ignore"):
        lum = tr.lum3(means[:, 0], means[:, 1], means[:, 2])
    for t in (edges, np.nextafter(edges, F(0)), np.nextafter(edges, F(np.inf))):
        assert np.isin(t, lum).all()  # every edge, the float below it and the float above it is some pixel's luminance
    got = api.luminance_histogram_host(means)
    counts, n_dark = tr.histogram(means)
    assert np.array_equal(api.luminance_counts(got), counts) and got.n_dark == n_dark and got.n_pixels == len(means) == n_dark + counts.sum()
    assert n_dark == 10 and (counts > 0).all()  # (the zeros, negatives, NaNs and -inf among the grey pixels; every bin is met)
    four = np.concatenate([means, np.full((len(means), 1), 9.0, np.float32)], -1)
    assert np.array_equal(api.luminance_counts(api.luminance_histogram_host(four)), counts)


def test_exposure_scale_is_exact_over_its_range(hip_lib):
    for e8 in range(tr.E8_MIN - 9, tr.E8_MAX + 10):
        got, want = api.exposure_scale(e8), tr.exposure_scale(e8)
        assert got == want and np.isfinite(got) and got >= np.finfo(np.float32).tiny, e8
    assert api.exposure_scale(0) == 1 and api.exposure_scale(8) == 2 and api.exposure_scale(-8) == 0.5 and api.exposure_scale(-1) == F(2 ** (7 / 8)) / 2
    assert api.exposure_scale(3) == F(2 ** (3 / 8)) and api.exposure_scale(-24) == F(2 ** -3)
    assert api.exposure_scale(10 ** 6) == api.exposure_scale(tr.E8_MAX) and api.exposure_scale(-10 ** 6) == api.exposure_scale(tr.E8_MIN)
    assert [api.exposure_e8(ev) for ev in (0, 1.5, -2.5, 0.0624, 0.0625, -0.0625, 0.07)] == [0, 12, -20, 0, 1, 0, 1]


def test_auto_exposure_integers_on_crafted_histograms(hip_lib):
    def check(counts, key=-20):
        s = stats_of(counts)
        assert api.luminance_mean_bin_x256(s) == tr.mean_bin_x256(counts)
        for p in (0, 1, 500, 900, 999, 1000):
            assert api.luminance_percentile_bin(s, p) == tr.percentile_bin(counts, p), p
        assert api.auto_exposure_e8(s, key) == tr.auto_exposure_e8(counts, key)
        return api.auto_exposure_e8(s, key)

    one = np.zeros(256, np.uint64)
    one[160] = 12345  # every pixel in [1, 1.09): the mean bin is 160.5, rounded to 161
    assert tr.mean_bin_x256(one) == 160 * 256 + 128 and check(one) == -20 + 160 - 161 == -21
    assert check(one, 0) == -1
    two = np.zeros(256, np.uint64)
    two[100], two[140] = 3, 1  # (3 x 201 + 281) x 128 / 4 = 28288: bin 110.5
    assert tr.mean_bin_x256(two) == 28288 and check(two) == -20 + 160 - 111
    assert tr.percentile_bin(two, 750) == 100 and tr.percentile_bin(two, 751) == 140 and tr.percentile_bin(two, 0) == 0
    big = np.zeros(256, np.uint64)
    big[0], big[255] = 0xffffffff, 0xffffffff  # the sums need 64 bits
    assert check(big) == -20 + 160 - 128
    empty = np.zeros(256, np.uint64)
    s = stats_of(empty, n_dark=77)
    assert api.auto_exposure_e8(s) == 0 == tr.auto_exposure_e8(empty) and api.luminance_mean_bin_x256(s) == 0 and api.luminance_percentile_bin(s, 500) == -1
    bright = np.zeros(256, np.uint64)
    bright[255] = 1
    assert check(bright, 2000) == tr.E8_MAX and check(one, -2000) == tr.E8_MIN  # held to the range of rene_exposure_scale
    rng = np.random.default_rng(5)
    for _ in range(20):
        check(rng.integers(0, 1 << 20, 256).astype(np.uint64) * (rng.random(256) < 0.3), int(rng.integers(-60, 20)))
    # shards add up
    parts = [stats_of(rng.integers(0, 1000, 256), n_dark=int(rng.integers(0, 50))) for _ in range(3)]
    total = api.luminance_combine(parts)
    assert np.array_equal(api.luminance_counts(total), sum(api.luminance_counts(p) for p in parts))
    assert total.n_dark == sum(p.n_dark for p in parts) and total.n_pixels == sum(p.n_pixels for p in parts) and total.struct_size == C.sizeof(total)
    bad = stats_of(one)
    bad.struct_size = 8
    with pytest.raises(api.ReneError):
        api.luminance_combine([parts[0], bad])
    with pytest.raises(api.ReneError):
        api.luminance_combine([stats_of(big), stats_of(big)])  # beyond uint32


def test_the_units_are_built_with_the_robust_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    variant = mk[mk.index("\nvariant:"):mk.index("\nclean:")]
    for unit in ("kernels_tonemap", "kernels_luminance"):
        assert unit + ".o" in objs
        rule = re.search(rf"^{unit}\.o: {unit}\.hip \$\(HDRS\)\n\t(.*)$", mk, re.M).group(1)
        assert "$(ROBUSTFLAGS)" in rule and "$(HIPFLAGS)" not in rule and "$(RESFLAGS)" in rule and f"2> {unit}.res" in rule
        assert re.search(rf"\$\(ROBUSTFLAGS\) \$\(RESFLAGS\) \$\(EXTRA\) -c -o var_\$\(NAME\)/{unit}\.o {unit}\.hip", variant)
    assert "output_pixel.h" in re.search(r"^HDRS = (.*)$", mk, re.M).group(1).split()


def _kernels(unit):
    text = open(os.path.join(CSRC, unit + ".res")).read()
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", text, re.S):
        g = lambda key: int(re.search(re.escape(key) + r": (\d+)", m.group(2)).group(1))
        out[m.group(1)] = {"scratch": g("ScratchSize [bytes/lane]"), "occupancy": g("Occupancy [waves/SIMD]"), "sgpr_spill": g("SGPRs Spill"),
                           "vgpr_spill": g("VGPRs Spill"), "lds": int(m.group(3))}
    return out


def test_every_kernel_is_there_without_scratch_or_spills(hip_lib):
    tm, lum = _kernels("kernels_tonemap"), _kernels("kernels_luminance")
    image = {re.search(r"tonemap_kernelILi(\d)ELi(\d)EE", n).groups() for n in tm if "tonemap_kernel" in n}
    probe = {re.search(r"tonemap_probe_kernelILi(\d)EE", n).group(1) for n in tm if "tonemap_probe_kernel" in n}
    assert image == {(o, f) for o in "012" for f in "01"} and probe == set("012") and len(tm) == 9, list(tm)
    assert len(lum) == 2 and any("luminance_kernel" in n for n in lum) and any("luminance_sum_kernel" in n for n in lum), list(lum)
    for name, k in {**tm, **lum}.items():
        assert k["scratch"] == 0 and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0 and k["occupancy"] >= 4, (name, k)
        if "tonemap" in name:
            assert k["lds"] == 1024, (name, k)  # the 255 thresholds, padded to 256 floats
        elif "luminance_kernel" in name:
            assert k["lds"] == 4 * 256 * 4 + 16, (name, k)  # one histogram per wave, and the waves' dark counts
        else:
            assert k["lds"] == 4 * 257 * 4, (name, k)  # the sum's four partial rows
