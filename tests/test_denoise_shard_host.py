"""CPU: the host surface of the denoiser on tile shards (rene_denoise_shard_* / rene_denoise_place_shard / rene_denoise_placed /
rene_gather_denoise, include/rene_hip.h): the size of a packed buffer restated in numpy, the header's layout as a ctypes mirror against the C
header, the exported symbols, and the argument checks that need no GPU."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT
from rene_amd import abi, api

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")

HEADER = os.path.join(ROOT, "include", "rene_hip.h")
TILE, SLOTS = 32, 1024
BYTES_PER_SLOT = 16 + 32 + 4  # the record, the two guide records, the variance plane
NEW_SYMBOLS = ("rene_denoise_shard_bytes", "rene_denoise_shard_prepare", "rene_denoise_shard_buffer", "rene_download_denoise_shard",
               "rene_denoise_place_shard", "rene_denoise_placed", "rene_gather_denoise")


def n_tiles(w, h):
    return -(-w // TILE) * -(-h // TILE)


def shard_bytes(w, h, rank, count):
    """include/rene_hip.h: header, one 8-byte entry per owned tile padded to 16 bytes, 52 bytes per slot of every owned tile."""
    owned = len(np.arange(n_tiles(w, h))[rank::count])
    return C.sizeof(abi.DenoiseShardHeader) + (owned * C.sizeof(abi.DenoiseShardTile) + 15) // 16 * 16 + owned * SLOTS * BYTES_PER_SLOT


@pytest.mark.parametrize("w,h,count", [(100, 70, 1), (100, 70, 2), (100, 70, 3), (100, 70, 5), (100, 70, 16), (161, 130, 3)])
def test_shard_bytes_is_its_restatement(hip_lib, w, h, count):
    sizes = [api.denoise_shard_bytes(w, h, r, count) for r in range(count)]
    assert sizes == [shard_bytes(w, h, r, count) for r in range(count)]
    assert all(s % 16 == 0 and s >= 64 for s in sizes)
    owned = [len(range(r, n_tiles(w, h), count)) for r in range(count)]
    overhead = sum(64 + (8 * o + 15) // 16 * 16 for o in owned)
    assert sum(sizes) == overhead + BYTES_PER_SLOT * SLOTS * n_tiles(w, h)  # the bodies together are the unsharded filter's records
    if count > n_tiles(w, h):
        assert sizes[-1] == 64  # a shard that owns nothing: a header
    assert abi.DENOISE_SHARD_TILE_BYTES == BYTES_PER_SLOT * SLOTS


def test_shard_bytes_refuses_what_is_no_shard(hip_lib):
    assert api.denoise_shard_bytes(100, 70) == shard_bytes(100, 70, 0, 1)
    for args in ((0, 70, 0, 1), (100, 0, 0, 1), (100, 70, 0, 0), (100, 70, 2, 2), (16385, 70, 0, 1)):
        assert api.denoise_shard_bytes(*args) == 0, args


def test_header_mirror_matches_the_c_header():
    fields = ("magic", "header_bytes", "width", "height", "shard_rank", "shard_count", "n_owned", "reserved", "params")
    prog = '#include <stdio.h>\n#include "rene_hip.h"\nint main(void){\n'
    prog += 'printf("header %zu\\ntile %zu\\n", sizeof(rene_denoise_shard_header), sizeof(rene_denoise_shard_tile));\n'
    for f in fields:
        prog += f'printf("{f} %zu\\n", offsetof(rene_denoise_shard_header, {f}));\n'
    prog += 'printf("valid %zu\\n", offsetof(rene_denoise_shard_tile, valid));\n'
    prog += 'printf("magic_value %u\\ntile_bytes %u\\n", RENE_DENOISE_SHARD_MAGIC, RENE_DENOISE_SHARD_TILE_BYTES);\nreturn 0;}\n'
    with tempfile.TemporaryDirectory() as d:  # the header still compiles as C99, as tests/test_abi.py compiles it
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), src, "-o", exe])
        out = {k: int(v) for k, v in (l.split() for l in subprocess.check_output([exe]).decode().splitlines())}
    assert out["header"] == C.sizeof(abi.DenoiseShardHeader) == 64 and out["tile"] == C.sizeof(abi.DenoiseShardTile) == 8
    for f in fields:
        assert out[f] == getattr(abi.DenoiseShardHeader, f).offset, f
    assert out["valid"] == abi.DenoiseShardTile.valid.offset == 4
    assert out["magic_value"] == abi.DENOISE_SHARD_MAGIC == int.from_bytes(b"DNSH", "little") and out["tile_bytes"] == abi.DENOISE_SHARD_TILE_BYTES
    assert np.dtype(abi.DENOISE_SHARD_TILE_DTYPE).itemsize == 8


def test_symbols_are_exported_and_additive(hip_lib):
    text = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert name in abi.EXPORTED_SYMBOLS and hasattr(hip_lib, name) and re.search(r"\b" + name + r"\(", text), name
        assert getattr(hip_lib, name).argtypes, name
    assert abi.ABI_VERSION == 7 and hip_lib.rene_abi_version() == 7 and C.sizeof(abi.DenoiseParams) == 32  # added symbols: nothing that existed moved
    for name in ("denoise_shard_prepare", "denoise_shard_buffer", "download_denoise_shard", "denoise_place_shard", "denoise_placed", "gather_denoise"):
        assert callable(getattr(api.Renderer, name)), name
    assert callable(api.denoise_shards) and callable(api.denoise_shard_bytes)


def test_null_arguments_are_refused_without_a_gpu(hip_lib):
    calls = {"rene_denoise_shard_prepare": (None, None), "rene_denoise_shard_buffer": (None, None, None), "rene_download_denoise_shard": (None, None, 0),
             "rene_denoise_place_shard": (None, None, 0), "rene_denoise_placed": (None,), "rene_gather_denoise": (None, 0)}
    for name, args in calls.items():
        assert getattr(hip_lib, name)(*args) == -1, name
        assert name.encode() in hip_lib.rene_last_error() and b"NULL" in hip_lib.rene_last_error(), name
    with pytest.raises(ValueError):
        api.denoise_shards([], via="carrier pigeon")


def test_cli_refuses_firefly_rejection_on_several_gpus(hip_lib):
    """The trimmed filter stays refused for tile shards, with a message that says the plain one is what the library offers them."""
    if not os.path.exists(CLI):
        api.build()
    for denoiser in ("atrous", "atrous-tiles"):
        for args in (["--gpus", "2", "--denoiser", denoiser, "--reject-fireflies"], ["--reject-gain", "0.5", "--denoiser", denoiser, "--gpus", "3"]):
            r = subprocess.run([CLI, *args, "x.pbrt"], capture_output=True, text=True)
            assert r.returncode == 2, (args, r.stderr)
            assert "--reject-fireflies cannot be combined with --gpus" in r.stderr and "plain filter" in r.stderr and "rene_denoise_shard_prepare" in r.stderr, r.stderr
    r = subprocess.run([CLI, "--denoiser", "atrous", "--reject-fireflies", str(os.path.join(ROOT, "missing.pbrt"))], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot be combined" not in r.stderr  # one GPU: past option parsing, the loader's error
