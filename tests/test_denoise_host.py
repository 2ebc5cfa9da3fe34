"""CPU: the `atrous` denoiser's host surface (command line, parameter defaults, argument checks) and its specification -- the numpy
restatement of tests/atrous_reference.py fed by the CPU oracle's renders: does the filter defined in include/rene_hip.h denoise, and is it
well enough conditioned in fp32 for a device implementation to be held to it?"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import atrous_reference as ar
from conftest import ROOT
from rene_amd import abi, api, scenes

CLI = os.path.join(ROOT, "rene_amd", "csrc", "rene-hip")
THREADS = 8


@pytest.fixture(scope="module")
def cli(hip_lib):
    if not os.path.exists(CLI):
        api.build()
    return CLI


def test_cli_accepts_atrous(cli, tmp_path):
    missing = str(tmp_path / "missing.pbrt")
    r = subprocess.run([cli, "--denoiser", "atrous", missing], capture_output=True, text=True)
    assert r.returncode == 1 and "invalid --denoiser" not in r.stderr, (r.returncode, r.stderr)  # past option parsing: the loader's error
    assert r.stdout.strip() and "denoiser was enabled" not in r.stderr
    r = subprocess.run([cli, "--denoiser", "atrous", "--gpus", "2", "x.pbrt"], capture_output=True, text=True)
    assert r.returncode == 2 and "--denoiser atrous" in r.stderr and "--gpus" in r.stderr, r.stderr
    r = subprocess.run([cli, "--gpus", "2", "--denoiser", "atrous", "x.pbrt"], capture_output=True, text=True)  # either order
    assert r.returncode == 2 and "--denoiser atrous" in r.stderr and "--gpus" in r.stderr, r.stderr
    r = subprocess.run([cli, "--denoiser", "bogus", "x.pbrt"], capture_output=True, text=True)
    assert r.returncode == 2 and "invalid --denoiser bogus" in r.stderr
    r = subprocess.run([cli, "--denoiser", "oidn", missing], capture_output=True, text=True)
    assert r.returncode == 1 and "WARN oidn denoiser was enabled but this build has no denoiser. Ignore." in r.stderr
    r = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert "none|optix|oidn|atrous" in r.stderr


def test_params_default_and_null_context(hip_lib):
    p = api.denoise_params_default()
    assert p.struct_size == C.sizeof(abi.DenoiseParams) == 32 and p.iterations == 5 and p.reserved == 0
    want = dict(sigma_luminance=4.0, sigma_normal2=1 / 64, sigma_albedo2=1 / 16, albedo_floor=0.05, relative_floor=1e-3)
    for k, v in want.items():
        assert getattr(p, k) == np.float32(v), k
        assert np.float32(ar.DEFAULTS[k]) == np.float32(v), k  # the restatement's defaults are the library's
    assert ar.DEFAULTS["iterations"] == p.iterations
    assert hip_lib.rene_denoise(None, None) == -1  # RENE_ERR_INVALID_ARGUMENT
    assert b"NULL context" in hip_lib.rene_last_error()
    buf = np.zeros(4, np.float32)
    assert hip_lib.rene_download_denoised(None, 0, 3, buf.ctypes.data_as(C.c_void_p), buf.size) == -1 and hip_lib.rene_last_error()
    ptr, n = C.c_void_p(), C.c_size_t()
    assert hip_lib.rene_denoised_buffer(None, C.byref(ptr), C.byref(n)) == -1 and hip_lib.rene_last_error()
    assert abi.ABI_VERSION == 7 and hip_lib.rene_abi_version() == 7


def test_params_struct_matches_the_header():
    import tempfile
    prog = ('#include <stdio.h>\n#include "rene_hip.h"\nint main(void){ printf("%zu %zu %u\\n", sizeof(rene_denoise_params), '
            'offsetof(rene_denoise_params, relative_floor), RENE_DENOISE_BYTES_PER_PIXEL); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        size, off, bpp = map(int, subprocess.check_output([exe]).split())
    assert size == C.sizeof(abi.DenoiseParams) and off == abi.DenoiseParams.relative_floor.offset and bpp == abi.DENOISE_BYTES_PER_PIXEL


# ---- the specification on oracle renders -----------------------------------------------------------------------------------------
CASES = {
    "cornell": (lambda: scenes.cornell_box(100, 70), 12),  # ragged tiles; chains of 2 and 1 frames
    "zoo": (lambda: scenes.material_zoo(192, 128), 32),
    "veach": (lambda: scenes.veach_mis(160, 90), 32),
    "fog": (lambda: scenes.cornell_fog(96, 64), 32),
}
REF_SPP = 2048


@pytest.fixture(scope="module")
def oracle_jobs(oracle_mod):
    jobs = {}

    def get(name):
        if name not in jobs:
            make, spp = CASES[name]
            o = oracle_mod.Oracle(make())
            o.render(100000, REF_SPP, threads=THREADS)
            ref = o.download(0).astype(np.float64) / REF_SPP
            jobs[name] = (ar.chains_of(o, spp, threads=THREADS), spp, ref)
        return jobs[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_denoises_oracle_renders(oracle_jobs, name):
    """relMSE(denoised) <= 0.5 relMSE(noisy) against an independent 2048-spp render (measured ratios 0.06 - 0.25: the margin is for another
    reference sample count or seed, not for the filter), and the fp32 run of the restatement stays within 4e-6 (1 + |value|) of the fp64 run
    (3 x the 1.3e-6 measured): the conditioning that justifies holding the device to 2e-5."""
    (chains, n_c, s1, s2), spp, ref = oracle_jobs(name)
    noisy = chains.astype(np.float64).sum(0) / spp
    out64, var64 = ar.denoise(chains, n_c, s1, s2)
    out32, _ = ar.denoise(chains, n_c, s1, s2, dtype=np.float32)
    assert out32.dtype == np.float32 and out64.dtype == np.float64
    e0, e1 = ar.relmse(noisy, ref), ar.relmse(out64 / spp, ref)
    spread = float((np.abs(out32 / np.float32(spp) - out64 / spp) / (1 + np.abs(out64 / spp))).max())
    print(f"{name}: relMSE noisy {e0:.4g} denoised {e1:.4g} ratio {e1 / e0:.3f}; mean ratio {out64.mean() / spp / noisy.mean():.3f}; fp32 vs fp64 {spread:.3g}")
    assert np.isfinite(out64).all() and (out64 >= 0).all() and (var64 >= 0).all()
    assert e1 <= 0.5 * e0, (name, e0, e1)
    assert spread <= 4e-6, (name, spread)


def test_constant_image_is_a_fixed_point():
    h, w = 37, 45
    rng = np.random.default_rng(5)
    colour, albedo, normal = rng.uniform(0.2, 2.0, 3), rng.uniform(0.1, 0.9, 3), np.array([0.0, 0.6, -0.8])
    n_c = np.full(8, 3.0)
    chains = np.broadcast_to(colour * 3.0, (8, h, w, 3)).astype(np.float32)
    s1 = np.broadcast_to(normal * 24.0, (h, w, 3)).astype(np.float32)
    s2 = np.broadcast_to(albedo * 24.0, (h, w, 3)).astype(np.float32)
    out, var = ar.denoise(chains, n_c, s1, s2)
    want = chains.astype(np.float64).sum(0)
    assert np.abs(out - want).max() <= 1e-6 * np.abs(want).max() and np.abs(var).max() <= 1e-12


def test_unequal_chains_give_finite_output(oracle_mod):
    o = oracle_mod.Oracle(scenes.cornell_box(40, 28))
    for spp, k in ((12, 8), (5, 5)):  # chains of 2 and 1 frames; five chains of one frame, three empty
        chains, n_c, s1, s2 = ar.chains_of(o, spp, threads=THREADS)
        assert int((n_c > 0).sum()) == k and n_c.sum() == spp
        for dt in (np.float64, np.float32):
            out, var = ar.denoise(chains, n_c, s1, s2, dtype=dt)
            assert np.isfinite(out).all() and (out >= 0).all() and np.isfinite(var).all() and (var >= 0).all()
        assert out.mean() > 0
