"""CPU: the host side of the compressed OpenEXR output (rene_exr_compress, include/rene_hip.h).  The device's bytes are held to
rene_exr_compress_host, so what is checked here, without a GPU, is that function: its tail byte for byte against the restatement of the
specification in tests/exr_zips_reference.py, the round trip through an independent reader that inflates with zlib, the library's own loader on a
written file, the attributes against the independent writer of tests/test_images.py, crafted bodies at every edge of the token rule, the refusals,
the command line's option, and a stand-alone program that runs the host code under AddressSanitizer and UndefinedBehaviorSanitizer."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import exr_reference as er
import exr_zips_reference as zr
from conftest import ROOT
from rene_amd import abi, api
from test_images import exr_bytes, load

CSRC = os.path.join(ROOT, "rene_amd", "csrc")
CLI = os.path.join(CSRC, "rene-hip")
CASES = zr.cpu_cases()
IDS = [c[0] for c in CASES]


def attr_bytes(w, h, mask):
    return api.exr_layout(w, h, mask)[0] - 8 * h


def test_constants_and_symbols(hip_lib):
    header = open(os.path.join(ROOT, "include", "rene_hip.h")).read()
    assert int(re.search(r"#define RENE_EXR_COMPRESSION_NONE (\d+)u", header).group(1)) == abi.EXR_COMPRESSION_NONE == 0
    assert int(re.search(r"#define RENE_EXR_COMPRESSION_ZIPS (\d+)u", header).group(1)) == abi.EXR_COMPRESSION_ZIPS == 2
    for sym in ("rene_exr_tail_bound", "rene_exr_attributes", "rene_exr_compress_host", "rene_exr_compress", "rene_exr_tail_buffer", "rene_download_exr_tail",
                "rene_output_exr_compressed", "rene_write_exr_compressed"):
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(hip_lib, sym) and re.search(rf"\b{sym}\(", header), sym
    assert re.search(r"#define RENE_ABI_VERSION 7u", header) and C.sizeof(abi.ExrParams) == 16  # added symbols only: the struct is what it was
    assert api.exr_tail_bound(23, 37, abi.EXR_ALL) == 8 * 37 + api.exr_layout(23, 37, abi.EXR_ALL)[1]
    assert api.exr_tail_bound(16384, 16384, abi.EXR_ALL) == 8 * 16384 + 16384 * (8 + 16384 * 66)


def test_the_segment_literal_is_the_kernels_constant():
    src = open(os.path.join(CSRC, "kernels_exr_zips.hip")).read()
    assert int(re.search(r"constexpr uint32_t EXR_ZIPS_SEGMENT = (\d+);", src).group(1)) == zr.SEGMENT


def test_the_unit_is_built_and_has_no_scratch(hip_lib):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "kernels_exr_zips.o" in re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    assert "exr_deflate.h" in re.search(r"^HDRS = (.*)$", mk, re.M).group(1).split()
    res = open(os.path.join(CSRC, "kernels_exr_zips.res")).read()
    kernels = re.findall(r"Function Name: (\S+)", res)
    assert len(kernels) == 3 and all(any(k in name for name in kernels) for k in ("zips_size_kernel", "zips_scan_kernel", "zips_encode_kernel"))
    assert set(re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res)) == {"0"}
    for unit in ("kernels_exr_zips.hip", "rene_hip.cpp"):  # one header for the code and the token rule
        assert '#include "exr_deflate.h"' in open(os.path.join(CSRC, unit)).read(), unit


@pytest.mark.parametrize("mask", [abi.EXR_BEAUTY, abi.EXR_DEFAULT, abi.EXR_IDS, abi.EXR_ALL])
def test_attributes_equal_the_independent_writers_header(hip_lib, mask):
    w, h = 7, 5
    zeros = {n: (np.zeros((h, w), {"half": np.float16, "float": np.float32, "uint": np.uint32}[t]), t) for n, b, t in abi.EXR_CHANNELS if mask & b}
    n = attr_bytes(w, h, mask)
    assert api.exr_attributes(w, h, mask, "zips") == exr_bytes(zeros, h, w, 2)[:n]
    assert api.exr_attributes(w, h, mask, "none") == api.exr_header(w, h, mask)[:n] == exr_bytes(zeros, h, w, 0)[:n]
    assert len(api.exr_attributes(w, h, mask, 2)) == n


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tail_is_the_specifications_bit_for_bit_and_reads_back(hip_lib, case):
    name, w, h, mask, body = case
    a = attr_bytes(w, h, mask)
    got = api.exr_compress_host(w, h, mask, body, "zips")
    want, stored, matches = zr.tail(w, h, mask, body, a)
    assert len(got) == len(want), (name, len(got), len(want))  # `written` is exact
    bad = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
    assert bad.size == 0, (name, bad[:8].tolist())
    table = struct.unpack_from(f"<{h}Q", got, 0)
    assert table[0] == a + 8 * h
    # the round trip: the independent reader follows every offset (and asserts the chunks are back to back and the file ends with the last)
    rw, rh, chans, compression, read_stored = zr.read(api.exr_attributes(w, h, mask, "zips") + got)
    assert (rw, rh, compression) == (w, h, 2) and read_stored == stored
    pw, ph, plain = er.parse(api.exr_header(w, h, mask) + body)
    assert list(chans) == list(plain)
    for ch in plain:
        assert np.array_equal(chans[ch].view(np.uint8), plain[ch].view(np.uint8)), (name, ch)
    # what each body is there for
    if name == "random rows":
        assert all(stored)
    if name in ("constant rows", "period 1 and period 2"):
        assert not any(stored)
    if name == "mixed rows":
        assert any(stored) and not all(stored)
    if name == "interval lengths":
        assert matches == [r // 258 + (r % 258 >= 3) for r in zr.INTERVAL_LENGTHS]
    if name == "1 x 1 alpha":
        assert stored == [True] and len(got) == 8 + 8 + 2  # n = 2: the stream is longer than the row


def test_no_compression_gives_the_present_file(hip_lib):
    for name, w, h, mask, body in CASES[:2] + CASES[-3:]:
        head = api.exr_header(w, h, mask)
        a = attr_bytes(w, h, mask)
        assert api.exr_compress_host(w, h, mask, body, "none") == head[a:] + body, name
        assert api.exr_attributes(w, h, mask, "none") == head[:a]


def test_the_librarys_loader_reads_a_compressed_file(hip_lib, tmp_path):
    w, h, mask = 23, 37, abi.EXR_BEAUTY | abi.EXR_ALPHA
    rng = np.random.default_rng(7)
    beauty = (rng.random((h, w, 3)) * 4).astype(np.float32)
    alpha = rng.random((h, w)).astype(np.float32)
    beauty[:12], alpha[:20] = np.float32(0.25), np.float32(1.0)  # rows that compress, rows that do not, rows of both kinds of channel
    body = api.exr_body_host(w, h, mask, beauty=beauty, alpha=alpha)
    tail = api.exr_compress_host(w, h, mask, body, "zips")
    stored = zr.read(api.exr_attributes(w, h, mask, "zips") + tail)[4]
    assert any(stored) and not all(stored)
    (tmp_path / "ba.exr").write_bytes(api.exr_attributes(w, h, mask, "zips") + tail)
    got = load(tmp_path, "ba.exr").reshape(h, w, 4)
    want = np.concatenate([er.half(beauty), er.half(alpha)[..., None]], axis=-1).astype(np.float32)
    assert np.array_equal(got, want)


def test_refusals_without_a_gpu(hip_lib):
    L = hip_lib
    w, h, mask = 4, 4, abi.EXR_BEAUTY
    body_bytes, bound = api.exr_layout(w, h, mask)[1], api.exr_tail_bound(w, h, mask)
    body, dst, written = C.create_string_buffer(body_bytes), C.create_string_buffer(bound), C.c_size_t(77)
    ok = lambda *a: L.rene_exr_compress_host(*a)
    assert ok(w, h, mask, 2, body, body_bytes, dst, bound, C.byref(written)) == 0
    before = dst.raw
    written.value = 77
    for compression in (1, 3, 4, 255):
        assert ok(w, h, mask, compression, body, body_bytes, dst, bound, C.byref(written)) == -1 and b"compression" in L.rene_last_error(), compression
        buf = C.create_string_buffer(1024)
        assert L.rene_exr_attributes(w, h, mask, compression, buf, 1024) == -1, compression
        assert L.rene_exr_compress(None, w, h, mask, compression, body, body_bytes, None, 0, C.byref(written)) == -1
    for bad in (body_bytes - 1, body_bytes + 1, 0):
        assert ok(w, h, mask, 2, body, bad, dst, bound, C.byref(written)) == -1 and b"body_bytes" in L.rene_last_error(), bad
    assert ok(w, h, mask, 2, body, body_bytes, dst, bound - 1, C.byref(written)) == -1 and b"dst_bytes" in L.rene_last_error()
    assert ok(w, h, mask, 2, None, body_bytes, dst, bound, C.byref(written)) == -1
    assert ok(w, h, mask, 2, body, body_bytes, None, bound, C.byref(written)) == -1
    assert ok(w, h, mask, 2, body, body_bytes, dst, bound, None) == -1
    for bw, bh, bm in ((0, 4, 1), (4, 0, 1), (16385, 4, 1), (4, 4, 0), (4, 4, 256)):
        assert ok(bw, bh, bm, 2, body, body_bytes, dst, bound, C.byref(written)) == -1, (bw, bh, bm)
        assert L.rene_exr_tail_bound(bw, bh, bm) == 0
    assert written.value == 77 and dst.raw == before  # a refused call writes nothing
    n = attr_bytes(w, h, mask)
    buf = C.create_string_buffer(n)
    assert L.rene_exr_attributes(w, h, mask, 2, buf, n) == 0
    assert L.rene_exr_attributes(w, h, mask, 2, buf, n - 1) == -1 and b"dst_bytes" in L.rene_last_error()
    assert L.rene_exr_attributes(w, h, mask, 2, None, n) == -1
    # the calls that need a context
    p = api.exr_params_default()
    assert L.rene_exr_compress(None, w, h, mask, 2, body, body_bytes, None, 0, C.byref(written)) == -1 and b"NULL context" in L.rene_last_error()
    assert L.rene_output_exr_compressed(None, C.byref(p), 2, None, 0, C.byref(written)) == -1 and b"NULL context" in L.rene_last_error()
    assert L.rene_write_exr_compressed(None, C.byref(p), 2, b"x.exr") == -1
    ptr, nb = C.c_void_p(), C.c_size_t()
    assert L.rene_exr_tail_buffer(None, C.byref(ptr), C.byref(nb)) == -1 and L.rene_download_exr_tail(None, None, 0) == -1
    with pytest.raises(ValueError):
        api.exr_compression("zip")
    assert api.exr_compression("zips") == 2 and api.exr_compression("none") == 0


def test_cli_option(hip_lib, tmp_path):
    if not os.path.exists(CLI):
        api.build()
    run = lambda *a: subprocess.run([CLI, *a], capture_output=True, text=True, cwd=tmp_path)
    missing = str(tmp_path / "missing.pbrt")
    assert "--exr-compression none|zips" in run("--help").stderr
    for value in ("none", "zips"):  # the option parses: the run gets as far as the scene file
        r = run(missing, "--exr", "o.exr", "--exr-compression", value)
        assert r.returncode == 1 and "cannot open" in r.stdout and "unknown option" not in r.stderr, (value, r.stderr)
    r = run(missing, "--exr", "o.exr", "--exr-compression", "zip")
    assert r.returncode == 2 and "unknown compression 'zip'" in r.stderr
    r = run(missing, "--exr-compression", "zips")
    assert r.returncode == 2 and "needs --exr" in r.stderr


def test_host_code_under_the_sanitizers(hip_lib, tmp_path):
    """selftest/exr_zips_check: some hundreds of random and crafted bodies through rene_exr_compress_host, every chunk inflated with zlib's
    uncompress and compared with the body -- a program of its own, its host code built with -fsanitize=address,undefined."""
    program = os.path.join(CSRC, "selftest", "exr_zips_check_asan")
    if not os.path.exists(program):  # (part of `make all`, so the build has left it there)
        subprocess.run(["make", "-C", CSRC, "selftest/exr_zips_check_asan"], check=True, capture_output=True)
    r = subprocess.run([program], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
