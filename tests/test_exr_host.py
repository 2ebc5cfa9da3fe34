"""CPU: the host side of the multi-channel OpenEXR output (rene_output_exr, include/rene_hip.h).  The device's bytes are held to
rene_exr_body_host, so what is checked here, without a GPU, is that function and rene_exr_header against an independent writer
(tests/test_images.py's exr_bytes) byte for byte, the library's own decoder on such a file, rene_exr_layout for every mask, the refusals that need
no device and the command line's options."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import exr_reference as er
from conftest import ROOT
from rene_amd import abi, api
from test_images import exr_bytes, load

CSRC = os.path.join(ROOT, "rene_amd", "csrc")
CLI = os.path.join(CSRC, "rene-hip")
SIZES = [(1, 1), (2, 3), (23, 37), (77, 45)]  # W x H
MASKS = [abi.EXR_BEAUTY, abi.EXR_DEFAULT, abi.EXR_BEAUTY | abi.EXR_DEPTH, abi.EXR_BEAUTY | abi.EXR_ALPHA, abi.EXR_IDS, abi.EXR_ALPHA | abi.EXR_POSITION | abi.EXR_NORMAL,
         abi.EXR_DENOISED | abi.EXR_IDS | abi.EXR_DEPTH, abi.EXR_ALL]
CASES = [(w, h, m) for w, h in SIZES for m in MASKS]


def planes(w, h, seed):
    """Random planes with the edge values scattered through every float plane."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in (("beauty", (h, w, 3)), ("albedo", (h, w, 3)), ("normal", (h, w, 3)), ("denoised", (h, w, 3)), ("alpha", (h, w)), ("depth", (h, w)),
                        ("position", (h, w, 3)), ("coverage", (h, w, 4))):
        a = (rng.standard_normal(shape) * np.exp(rng.uniform(-18, 12, shape))).astype(np.float32)
        flat = a.reshape(-1)
        at = rng.choice(flat.size, min(flat.size, 4 * er.EDGE_VALUES.size), replace=flat.size < 4 * er.EDGE_VALUES.size)
        flat[at] = np.resize(er.EDGE_VALUES, at.size)
        out[name] = a
    out["ids"] = rng.integers(0, 1 << 32, (h, w, 4), dtype=np.uint64).astype(np.uint32)
    return out


def library_file(w, h, mask, pl):
    return api.exr_header(w, h, mask) + api.exr_body_host(w, h, mask, **pl)


def float_row_offset(w, mask):
    """Where the first FLOAT or UINT channel's row starts in row 0's chunk."""
    off = 8
    for name, bit, typ in abi.EXR_CHANNELS:
        if mask & bit:
            if typ != "half":
                return off
            off += 2 * w
    return None


def test_struct_defaults_and_symbols(hip_lib):
    p = api.exr_params_default()
    assert (p.struct_size, p.layers, p.beauty_source, p.reserved) == (C.sizeof(abi.ExrParams), abi.EXR_BEAUTY | abi.EXR_ALBEDO | abi.EXR_NORMAL, abi.OUTPUT_RADIANCE, 0)
    assert p.struct_size == 16 and C.sizeof(abi.ExrPlanes) == 8 + 9 * C.sizeof(C.c_void_p)
    header = open(os.path.join(ROOT, "include", "rene_hip.h")).read()
    for name in ("BEAUTY", "ALBEDO", "NORMAL", "DENOISED", "ALPHA", "DEPTH", "POSITION", "IDS", "ALL", "MAX_SIZE"):
        assert int(re.search(rf"#define RENE_EXR_{name} (\d+)u", header).group(1)) == getattr(abi, "EXR_" + name), name
    for cls, struct in ((abi.ExrParams, "rene_exr_params"), (abi.ExrPlanes, "rene_exr_planes")):
        body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", header, re.S).group(1)
        fields = re.findall(r"^\s*(?:const )?\w+\*? (\w+);", body, re.M)
        assert fields == [f for f, _ in cls._fields_], struct
    for sym in ("rene_exr_params_default", "rene_exr_layout", "rene_exr_header", "rene_output_exr", "rene_exr_buffer", "rene_download_exr", "rene_write_exr",
                "rene_exr_body_host"):
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(hip_lib, sym), sym
    assert re.search(r"#define RENE_ABI_VERSION 7u", header)
    names = [n for n, _, _ in abi.EXR_CHANNELS]
    assert names == sorted(names) and len(names) == 25  # the order of Python's sorted() on the names


@pytest.mark.parametrize("w,h,mask", CASES)
def test_header_and_host_body_equal_the_independent_writer(hip_lib, w, h, mask):
    pl = planes(w, h, 1000 * w + mask)
    want = er.file_bytes(mask, h, w, **pl)
    got = library_file(w, h, mask, pl)
    assert len(got) == len(want)
    bad = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
    assert bad.size == 0, (w, h, mask, bad[:8].tolist())
    head, body, bpp = api.exr_layout(w, h, mask)
    assert head + body == len(want) and body == h * (8 + w * bpp)
    pw, ph, chans = er.parse(got)
    assert (pw, ph) == (w, h) and list(chans) == [n for n, b, _ in abi.EXR_CHANNELS if mask & b]


def test_the_misaligned_float_row_is_among_the_cases(hip_lib):
    assert (77, 45, abi.EXR_BEAUTY | abi.EXR_DEPTH) in CASES
    off = float_row_offset(77, abi.EXR_BEAUTY | abi.EXR_DEPTH)
    assert off == 8 + 3 * 2 * 77 and off % 4 == 2  # Z follows B, G and R: row 0's FLOAT row starts at an address = 2 (mod 4)
    assert float_row_offset(77, abi.EXR_ALL) % 4 == 2  # (... and the P rows behind A, B, G)
    _, _, bpp = api.exr_layout(77, 45, abi.EXR_BEAUTY | abi.EXR_DEPTH)
    assert bpp == 10 and (8 + 77 * bpp) % 4 == 2  # the rows themselves alternate between the two alignments


def test_edge_values_become_the_halves_of_the_rule(hip_lib):
    v = er.EDGE_VALUES
    w = v.size
    rgb = np.stack([v, -v, v[::-1]], axis=-1)[None]
    body = api.exr_body_host(w, 1, abi.EXR_BEAUTY, beauty=rgb)
    got = np.frombuffer(body, "<f2", 3 * w, 8).reshape(3, w)  # B G R
    want = er.half(rgb[0].T[::-1])
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    r = got[2]
    assert np.isfinite(r[~np.isnan(v)]).all() and np.isnan(r[np.isnan(v)]).all()  # no infinity: clamped
    assert r[v == 65505.0][0] == 65504 and r[np.isposinf(v)][0] == 65504 and r[np.isneginf(v)][0] == -65504
    assert r[v == np.float32(3 * 2.0 ** -24)].view(np.uint16)[0] == 3  # a half subnormal, kept
    assert r[np.signbit(v) & (v == 0)].view(np.uint16)[0] == 0x8000  # -0.0


def test_the_librarys_decoder_reads_the_file(hip_lib, tmp_path):
    w, h, mask = 23, 37, abi.EXR_BEAUTY | abi.EXR_ALPHA
    rng = np.random.default_rng(7)
    beauty = (rng.random((h, w, 3)) * 4).astype(np.float32)
    alpha = rng.random((h, w)).astype(np.float32)
    (tmp_path / "ba.exr").write_bytes(library_file(w, h, mask, dict(beauty=beauty, alpha=alpha)))
    got = load(tmp_path, "ba.exr").reshape(h, w, 4)
    want = np.concatenate([er.half(beauty), er.half(alpha)[..., None]], axis=-1).astype(np.float32)
    assert np.array_equal(got, want)


def test_layout_of_every_mask(hip_lib):
    w, h = 5, 3
    zeros = dict(beauty=np.zeros((h, w, 3), np.float32), alpha=np.zeros((h, w), np.float32), ids=np.zeros((h, w, 4), np.uint32), coverage=np.zeros((h, w, 4), np.float32))
    zeros.update(albedo=zeros["beauty"], normal=zeros["beauty"], denoised=zeros["beauty"], position=zeros["beauty"], depth=zeros["alpha"])
    for mask in range(1, 256):
        head, body, bpp = api.exr_layout(w, h, mask)
        want = er.file_bytes(mask, h, w, **zeros)
        assert bpp == sum(2 if t == "half" else 4 for _, b, t in abi.EXR_CHANNELS if mask & b)
        assert (head + body, body) == (len(want), h * (8 + w * bpp)), mask
        assert api.exr_header(w, h, mask) == want[:head], mask
    assert api.exr_layout(1920, 1080, abi.EXR_ALL)[2] == 66 and api.exr_layout(1920, 1080, abi.EXR_BEAUTY)[2] == 6
    assert api.exr_layout(16384, 16384, abi.EXR_ALL)[1] == 16384 * (8 + 16384 * 66)  # beyond 2^32


def test_refusals_without_a_gpu(hip_lib):
    L = hip_lib
    p = api.exr_params_default()
    assert L.rene_output_exr(None, C.byref(p), None, 0) == -1 and b"NULL context" in L.rene_last_error()
    assert L.rene_write_exr(None, C.byref(p), b"x.exr") == -1
    ptr, n = C.c_void_p(), C.c_size_t()
    assert L.rene_exr_buffer(None, C.byref(ptr), C.byref(n)) == -1
    assert L.rene_download_exr(None, None, 0) == -1
    for w, h, mask in ((0, 4, 1), (4, 0, 1), (16385, 4, 1), (4, 16385, 1), (4, 4, 0), (4, 4, 256), (4, 4, 0x80000001)):
        assert L.rene_exr_layout(w, h, mask, None, None, None) == -1 and L.rene_last_error(), (w, h, mask)
        buf = C.create_string_buffer(4096)
        assert L.rene_exr_header(w, h, mask, buf, 4096) == -1, (w, h, mask)
    assert L.rene_exr_layout(4, 4, 1, None, None, None) == 0  # (every pointer is optional)
    head = api.exr_layout(4, 4, 1)[0]
    buf = C.create_string_buffer(head)
    assert L.rene_exr_header(4, 4, 1, buf, head - 1) == -1 and b"dst_bytes" in L.rene_last_error()
    assert L.rene_exr_header(4, 4, 1, None, head) == -1
    # the host pack: a plane of a chosen layer that is missing, a short destination, a struct of another size
    beauty = np.zeros((4, 4, 3), np.float32)
    with pytest.raises(api.ReneError) as e:
        api.exr_body_host(4, 4, abi.EXR_BEAUTY | abi.EXR_DEPTH, beauty=beauty)
    assert e.value.code == -1 and "Z" in str(e.value)
    pl = abi.ExrPlanes()
    pl.struct_size, pl.beauty = C.sizeof(abi.ExrPlanes), beauty.ctypes.data
    body = api.exr_layout(4, 4, 1)[1]
    out = C.create_string_buffer(body)
    assert L.rene_exr_body_host(4, 4, 1, C.byref(pl), out, body) == 0
    assert L.rene_exr_body_host(4, 4, 1, C.byref(pl), out, body - 1) == -1 and b"dst_bytes" in L.rene_last_error()
    assert L.rene_exr_body_host(4, 4, 1, C.byref(pl), None, body) == -1 and L.rene_exr_body_host(4, 4, 1, None, out, body) == -1
    pl.struct_size -= 8
    assert L.rene_exr_body_host(4, 4, 1, C.byref(pl), out, body) == -1 and b"struct_size" in L.rene_last_error()
    with pytest.raises(ValueError):
        api.exr_mask(("beauty", "bogus"))
    with pytest.raises(ValueError):
        api._exr_params(("beauty",), "denoised")  # the sums of rene_denoise are no mean
    assert api.exr_mask(("beauty", "ids")) == abi.EXR_BEAUTY | abi.EXR_IDS and api.exr_mask("depth") == abi.EXR_DEPTH


def test_the_unit_is_built_with_the_robust_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "kernels_exr.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    rule = re.search(r"^kernels_exr\.o: kernels_exr\.hip \$\(HDRS\)\n\t(.*)$", mk, re.M).group(1)
    assert "$(ROBUSTFLAGS)" in rule and "$(HIPFLAGS)" not in rule and "$(RESFLAGS)" in rule and "2> kernels_exr.res" in rule
    assert "half_element.h" in re.search(r"^HDRS = (.*)$", mk, re.M).group(1).split()
    for unit in ("kernels_exr.hip", "kernels_features.hip"):  # one rule for the halves, in one header
        src = open(os.path.join(CSRC, unit)).read()
        assert '#include "half_element.h"' in src and "_Float16 to_element<_Float16>" not in src, unit


def test_the_kernel_has_no_scratch(hip_lib):
    res = open(os.path.join(CSRC, "kernels_exr.res")).read()
    kernels = re.findall(r"Function Name: (\S+)", res)
    assert len(kernels) == 1 and "exr_kernel" in kernels[0]  # one kernel for every combination of layers
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res) == ["0"] and re.findall(r"LDS Size \[bytes/block\]: (\d+)", res) == ["0"]


def test_cli_options(hip_lib, tmp_path):
    if not os.path.exists(CLI):
        api.build()
    run = lambda *a: subprocess.run([CLI, *a], capture_output=True, text=True, cwd=tmp_path)
    missing = str(tmp_path / "missing.pbrt")
    r = run("--help")
    assert "--exr PATH" in r.stderr and "--exr-layers" in r.stderr
    # the options parse: the run gets as far as the scene file
    for extra in ([], ["--exr-layers", "beauty"], ["--exr-layers", "beauty,albedo,normal,alpha,depth,position,ids"],
                  ["--exr-layers", "beauty,denoised", "--denoiser", "atrous"], ["--exr-layers", "denoised", "--denoiser", "atrous-tiles"], ["--out", "x.exr"]):
        r = run(missing, "--exr", "o.exr", *extra)
        assert r.returncode == 1 and "cannot open" in r.stdout and "unknown option" not in r.stderr, (extra, r.stderr)
    r = run(missing, "--exr", "o.exr", "--exr-layers", "beauty,colour")
    assert r.returncode == 2 and "unknown layer 'colour'" in r.stderr
    r = run(missing, "--exr", "o.exr", "--exr-layers", "beauty,")
    assert r.returncode == 2 and "unknown layer ''" in r.stderr
    r = run(missing, "--exr", "o.exr", "--exr-layers", "beauty,denoised")
    assert r.returncode == 2 and "denoised needs --denoiser atrous" in r.stderr
    r = run(missing, "--exr", "o.exr", "--exr-layers", "denoised", "--denoiser", "oidn")
    assert r.returncode == 2
    r = run(missing, "--exr-layers", "beauty")
    assert r.returncode == 2 and "needs --exr" in r.stderr
    r = run(missing, "--exr", "o.exr", "--gpus", "2")
    assert r.returncode == 2 and "--gpus" in r.stderr
    r = run(missing, "--exr")
    assert r.returncode == 2 and "needs a value" in r.stderr
    # --out x.exr is not --exr: the reference's line and its PNG stay (the line itself is printed behind the render: tests/test_gpu_exr.py)
    src = open(os.path.join(CSRC, "rene_cli.cpp")).read()
    assert src.count('"INFO .exr output is not yet supported. Save as .png\\n"') == 1 and 'filename += ".png";' in src
