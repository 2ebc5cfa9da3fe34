"""CPU: the host surface of adaptive sampling (include/rene_hip.h: rene_set_active_tiles, rene_tile_frames, rene_download_mean,
rene_noise_select_tiles) -- the tile selection against its numpy restatement (tests/adaptive_reference.py), the header as C99, the exported
symbols and their Python mirrors, and the command line's refusals."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import adaptive_reference as ar
from conftest import ROOT
from rene_amd import abi, api, scenes

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
NEW_SYMBOLS = ["rene_set_active_tiles", "rene_tile_frames", "rene_download_mean", "rene_noise_select_tiles"]


def _grid(rng, ty=5, tx=7):
    """Tile records of a 200 x 150 image (ragged on both sides) with noise around 0.2, one black tile and one tile without pixels."""
    n = np.full((ty, tx), 1024)
    n[-1, :] = 22 * 32
    n[:, -1] = 8 * 32
    n[-1, -1] = 22 * 8
    t = np.zeros((ty, tx), np.dtype(abi.NOISE_TILE_DTYPE))
    lum = rng.uniform(0.05, 2.0, (ty, tx))
    rel = rng.uniform(0.0, 0.4, (ty, tx))
    t["sum_lum"] = (lum * n).astype(np.float32)
    t["sum_var"] = ((rel * (lum + 0.01)) ** 2 * n).astype(np.float32)
    t["n_pixels"] = n
    t["sum_lum"][1, 2] = t["sum_var"][1, 2] = 0  # a black tile: noise 0
    t["n_pixels"][3, 4] = 0                      # a tile that was not estimated
    return t


@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_select_tiles_equals_the_restatement(hip_lib, dilate):
    rng = np.random.default_rng(5 + dilate)
    seen = set()
    for trial in range(12):
        t = _grid(rng)
        active = None if trial == 0 else (rng.uniform(size=t.shape) < 0.7).astype(np.uint8)  # tiles already inactive
        for target in (0.1, 0.2, 0.35):
            got = api.noise_select_tiles(t, active, target, dilate)
            want = ar.select_tiles(t["sum_var"], t["sum_lum"], t["n_pixels"], active, 0.01, target, dilate)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (trial, target)
            assert got[3, 4] == 0 and (active is None or not got[active == 0].any())  # no pixels: off; the set only shrinks
            if dilate == 0:
                assert got[1, 2] == 0  # the black tile is below every target
            seen.add(int(got.sum()))
    assert len(seen) > 3  # the cases are not all "everything" or "nothing"
    # a lone noisy tile keeps its neighbourhood of that radius alive -- where the neighbours are active and have pixels
    t = _grid(rng)
    t["sum_var"] = 0
    t["sum_var"][2, 3] = 1e3
    got = api.noise_select_tiles(t, None, 0.2, dilate)
    want = np.zeros(t.shape, np.uint8)
    want[2 - dilate:3 + dilate, 3 - dilate:4 + dilate] = 1
    want[3, 4] = 0
    assert np.array_equal(got, want)


def test_select_tiles_in_place_and_argument_errors(hip_lib):
    L = hip_lib
    t = _grid(np.random.default_rng(1))
    want = ar.select_tiles(t["sum_var"], t["sum_lum"], t["n_pixels"], None, 0.01, 0.2, 1)
    a = np.ones(t.shape, np.uint8)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    assert L.rene_noise_select_tiles(p(t), p(a), 7, 5, 0.01, 0.2, 1, p(a)) == 0 and np.array_equal(a, want)  # active_out may be active_in
    out = np.zeros(t.shape, np.uint8)
    bad = [(None, p(out), 7, 5, 0.01, 0.2, 1), (p(t), None, 7, 5, 0.01, 0.2, 1), (p(t), p(out), 0, 5, 0.01, 0.2, 1), (p(t), p(out), 7, 0, 0.01, 0.2, 1),
           (p(t), p(out), 7, 5, 0.01, 0.2, 3), (p(t), p(out), 7, 5, 0.0, 0.2, 1), (p(t), p(out), 7, 5, float("nan"), 0.2, 1),
           (p(t), p(out), 7, 5, 0.01, 0.0, 1), (p(t), p(out), 7, 5, 0.01, -1.0, 1), (p(t), p(out), 7, 5, 0.01, float("inf"), 1)]
    for tiles, o, tx, ty, floor, target, dilate in bad:
        assert L.rene_noise_select_tiles(tiles, None, tx, ty, floor, target, dilate, o) == -1, (tx, ty, floor, target, dilate)
        assert L.rene_last_error().startswith(b"rene_noise_select_tiles: ")
    with pytest.raises(ValueError):
        api.noise_select_tiles(t, np.ones((2, 2)), 0.2)


def test_header_compiles_as_c99_with_the_new_declarations():
    """The declarations have the types a C caller expects (an assignment to a function pointer of that type compiles without a warning), and
    the ABI version is still 7: added symbols only."""
    typed = ('#include "rene_hip.h"\n'
             "int (*a)(rene_ctx*, const uint8_t*, size_t) = rene_set_active_tiles;\n"
             "int (*b)(rene_ctx*, uint32_t*, size_t) = rene_tile_frames;\n"
             "int (*c)(rene_ctx*, int, int, float*, size_t) = rene_download_mean;\n"
             "int (*d)(const rene_noise_tile*, const uint8_t*, uint32_t, uint32_t, float, double, uint32_t, uint8_t*) = rene_noise_select_tiles;\n")
    prints = '#include <stdio.h>\n#include "rene_hip.h"\nint main(void){printf("%u\\n", RENE_ABI_VERSION);return 0;}\n'
    gcc = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "typed.c"), "w").write(typed)
        open(os.path.join(d, "prints.c"), "w").write(prints)
        subprocess.check_call(gcc + ["-c", os.path.join(d, "typed.c"), "-o", os.path.join(d, "typed.o")])
        subprocess.check_call(gcc + [os.path.join(d, "prints.c"), "-o", os.path.join(d, "prints")])
        assert subprocess.check_output([os.path.join(d, "prints")]).split() == [b"7"]


def test_new_symbols_are_exported_and_mirrored(hip_lib):
    header = open(os.path.join(ROOT, "include", "rene_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in abi.EXPORTED_SYMBOLS, name
        assert getattr(hip_lib, name).argtypes, name  # the ctypes prototype is declared
    assert hip_lib.rene_abi_version() == abi.ABI_VERSION == 7
    for method in ("set_active_tiles", "tile_frames", "download_mean", "render_adaptive"):
        assert callable(getattr(api.Renderer, method))
    assert callable(api.noise_select_tiles)


def test_device_calls_without_a_context_or_a_gpu(hip_lib):
    """The library loads without a GPU; a context cannot exist there (rene_create: RENE_ERR_DEVICE, no CPU fallback), and the new device calls
    refuse a NULL context with a message."""
    L = hip_lib
    buf = np.zeros(64, np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    for rc in (L.rene_set_active_tiles(None, p, 64), L.rene_tile_frames(None, p, 64), L.rene_download_mean(None, 0, 3, p, 64)):
        assert rc == -1 and L.rene_last_error()
    from conftest import has_gpu
    if not has_gpu():
        with pytest.raises(api.ReneError) as e:
            api.Renderer(scenes.cornell_box(16, 16))
        assert e.value.code == -3  # RENE_ERR_DEVICE


def test_render_adaptive_checks_its_arguments_before_it_renders():
    class Never(api.Renderer):
        def __init__(self):
            pass

        def render(self, *a):
            raise AssertionError("rendered")

    for kw in (dict(batch=8), dict(batch=20), dict(target=0.0), dict(max_frames=1)):
        args = dict(target=0.1, max_frames=64)
        args.update(kw)
        with pytest.raises(ValueError):
            Never().render_adaptive(**args)


def test_cli_refuses_adaptive_combinations(hip_lib):
    if not os.path.exists(CLI):
        api.build()
    for args, word in ((["--adaptive"], "--target-noise"),
                       (["--adaptive", "--target-noise", "0.1", "--gpus", "2"], "--gpus"),
                       (["--adaptive", "--target-noise", "0.1", "--denoiser", "atrous"], "atrous"),
                       (["--adaptive", "--target-noise", "0.1", "--dilate", "3"], "--dilate")):
        r = subprocess.run([CLI, "x.pbrt"] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "rene-hip: " in r.stderr and word in r.stderr and "--adaptive" in r.stderr + " ".join(args), (args, r.stderr)
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--adaptive" in r.stderr and "--sample-map" in r.stderr and "--dilate" in r.stderr
