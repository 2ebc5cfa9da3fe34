"""CPU: the firefly-robust resolve's host surface (structs, defaults, the pure host function, argument checks) and its specification -- the numpy
restatement of tests/robust_reference.py on cases with a closed form and on the CPU oracle's renders: does the rule of include/rene_hip.h remove
the fireflies, and does the energy it removes come back as frames grow?"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import robust_reference as rr
from atrous_reference import relmse
from conftest import ROOT
from rene_amd import abi, api, scenes

THREADS = 8
REF_FRAMES, REF_FIRST = 1024, 100000  # the reference render: frames no job under test uses


def test_structs_match_the_header():
    fields = [("rene_robust_params", "max_trim"), ("rene_robust_params", "gain"), ("rene_robust_tile", "sum_lum_robust"), ("rene_robust_tile", "n_trimmed"),
              ("rene_robust_summary", "n_pixels"), ("rene_robust_summary", "n_trimmed"), ("rene_robust_summary", "sum_lum_plain"),
              ("rene_robust_summary", "kept_energy"), ("rene_robust_summary", "n_frames"), ("rene_robust_summary", "max_trim"), ("rene_robust_summary", "gain")]
    structs = ("rene_robust_params", "rene_robust_tile", "rene_robust_summary")
    prog = '#include <stdio.h>\n#include "rene_hip.h"\nint main(void){\n'
    for s in structs:
        prog += f'printf("%zu\\n", sizeof({s}));\n'
    for s, f in fields:
        prog += f'printf("%zu\\n", offsetof({s}, {f}));\n'
    prog += 'printf("%d %d\\n", RENE_ROBUST_IMAGE, RENE_ROBUST_TRIM);\nprintf("%u\\n", RENE_ABI_VERSION);\nreturn 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = list(map(int, subprocess.check_output([exe]).split()))
    cls = dict(zip(structs, (abi.RobustParams, abi.RobustTile, abi.RobustSummary)))
    assert out[:3] == [C.sizeof(abi.RobustParams), C.sizeof(abi.RobustTile), C.sizeof(abi.RobustSummary)] == [16, 16, 64]
    for got, (s, f) in zip(out[3:], fields):
        assert got == getattr(cls[s], f).offset, (s, f)
    assert out[-3:-1] == [abi.ROBUST_IMAGE, abi.ROBUST_TRIM] == [0, 1]
    assert out[-1] == abi.ABI_VERSION == 7  # new symbols and struct_size-carrying structs break no caller
    assert np.dtype(abi.ROBUST_TILE_DTYPE).itemsize == C.sizeof(abi.RobustTile)
    for name in ("rene_robust_params_default", "rene_resolve_robust", "rene_download_robust", "rene_download_robust_tiles", "rene_robust_combine"):
        assert name in abi.EXPORTED_SYMBOLS


def test_defaults_and_null_arguments(hip_lib):
    p = api.robust_params_default()
    assert p.struct_size == C.sizeof(abi.RobustParams) == 16 and p.reserved == 0
    assert p.max_trim == 3 == rr.DEFAULT_MAX_TRIM and p.gain == 1.0 == rr.DEFAULT_GAIN
    out = abi.RobustSummary()
    assert hip_lib.rene_resolve_robust(None, None, C.byref(out)) == -1 and b"NULL context" in hip_lib.rene_last_error()
    buf = (C.c_float * 4)()
    assert hip_lib.rene_download_robust(None, 0, 3, buf, 4) == -1 and hip_lib.rene_last_error()
    tiles = (abi.RobustTile * 4)()
    assert hip_lib.rene_download_robust_tiles(None, tiles, 4) == -1 and hip_lib.rene_last_error()
    assert hip_lib.rene_robust_combine(None, 0, C.byref(out)) == -1 and hip_lib.rene_last_error()
    assert hip_lib.rene_abi_version() == 7


# ---- closed forms on the restatement ------------------------------------------------------------------------------------------------
def _flat(means, n_c, h=3, w=5):
    """Chains whose means are means[c] in every channel and pixel (lum's weights add up to one: l_c = means[c])."""
    return np.stack([np.full((h, w, 3), float(n_c[c]) * means[c]) for c in range(8)])


def test_equal_chains_trim_nothing():
    n_c = np.full(8, 4)
    for dtype in (np.float64, np.float32):
        out = rr.resolve(_flat([0.75] * 8, n_c), n_c, dtype=dtype)
        assert (out["G"] == 0).all() and (out["j"] == 0).all()
        assert np.array_equal(out["image"], out["plain"]) and np.allclose(out["image"], 0.75, rtol=1e-6)


def test_one_firefly_chain_is_trimmed():
    """Means (1, 1, 1, 1, 1, 1, 1, 50): ranks 0 .. 7, num = sum (2 r + 1 - 8) l = -7 - 5 - 3 - 1 + 1 + 3 + 5 + 7 * 50 = 343, tot = 57,
    G = 343 / (8 * 57) = 343 / 456 = 0.752, t = 4 G = 3.009: j = 3, chains of rank 3 and 4 are kept, both of mean 1."""
    n_c = np.full(8, 2)
    means = [1.0] * 7 + [50.0]
    out = rr.resolve(_flat(means, n_c), n_c)
    assert np.abs(out["G"] - 343 / 456).max() <= 1e-12 and (out["j"] == 3).all()
    assert np.abs(out["image"] - 1.0).max() <= 1e-12 and np.abs(out["plain"] - 57 / 8).max() <= 1e-12
    out32 = rr.resolve(_flat(means, n_c), n_c, dtype=np.float32)
    assert out32["image"].dtype == np.float32 and (out32["j"] == 3).all() and (out32["image"] == 1).all()
    # the firefly in chain 2 instead: the same G, and the kept chains are again ordinary ones
    means = [1.0, 1.0, 50.0] + [1.0] * 5
    out = rr.resolve(_flat(means, n_c), n_c)
    assert np.abs(out["G"] - 343 / 456).max() <= 1e-12 and (out["j"] == 3).all() and np.abs(out["image"] - 1.0).max() <= 1e-12


def test_max_trim_and_gain_act_as_stated():
    n_c = np.full(8, 2)
    chains = _flat([1.0] * 7 + [50.0], n_c)
    for m in (0, 1, 2, 3):
        out = rr.resolve(chains, n_c, max_trim=m)
        assert (out["j"] == m).all()
        kept = 8 - 2 * m  # the m lowest are 1s, the m highest the 50 and m - 1 ones
        want = (57.0 - (2 * m - 1 + 50 if m else 0)) / kept
        assert np.abs(out["image"] - want).max() <= 1e-12, m
    assert np.array_equal(rr.resolve(chains, n_c, max_trim=0)["image"], rr.resolve(chains, n_c)["plain"])
    # t = gain * G * 4 with G = 0.752: gain 0.5 -> 1.504 -> 1; gain 0.3 -> 0.90 -> 0; gain 0.7 -> 2.1 -> 2; gain 10 -> capped at 3
    for gain, j in ((0.5, 1), (0.3, 0), (0.7, 2), (10.0, 3)):
        assert (rr.resolve(chains, n_c, gain=gain)["j"] == j).all(), gain


def test_five_frames_cap_the_trim_at_two():
    n_c = rr.chain_counts(5)
    assert n_c.tolist() == [1, 1, 1, 1, 1, 0, 0, 0]
    means = [1.0, 1.0, 400.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    out = rr.resolve(_flat(means, n_c), n_c)
    # G = (-4 - 2 + 0 + 2 + 4 * 400) / (5 * 404) = 0.79, t = 0.79 * 2.5 = 1.98 -> 1; with gain 4 t = 7.9, capped by (5 - 1) / 2 = 2
    assert (out["j"] == 1).all()
    out = rr.resolve(_flat(means, n_c), n_c, gain=4.0)
    assert (out["j"] == 2).all() and np.abs(out["image"] - 1.0).max() <= 1e-12  # one chain is left: the median
    # k = 2: (k - 1) / 2 = 0, nothing can be trimmed; k = 1 likewise
    for spp in (1, 2):
        n_c = rr.chain_counts(spp)
        out = rr.resolve(_flat([1.0, 90.0] + [0.0] * 6, n_c), n_c, gain=100.0)
        assert (out["j"] == 0).all() and np.array_equal(out["image"], out["plain"])


def test_ties_are_broken_by_chain_index():
    """Means (2, 2, 2, 2, 9, 9, 9, 9) with a large gain: j = 3 keeps ranks 3 and 4 -- chain 3 (the last of the 2s) and chain 4 (the first of the
    9s) by the tie rule; with unequal frame counts the result says which chains they were."""
    n_c = np.array([1, 1, 1, 3, 2, 1, 1, 1])
    means = [2.0] * 4 + [9.0] * 4
    out = rr.resolve(_flat(means, n_c), n_c, gain=100.0)
    assert (out["j"] == 3).all()
    assert np.abs(out["image"] - (3 * 2.0 + 2 * 9.0) / 5).max() <= 1e-12  # chains 3 and 4: five frames
    l = np.array(means)[:, None]
    rank, _ = rr.gini(l, np.float64)
    assert rank[:, 0].tolist() == list(range(8))


def test_black_pixel_and_no_frames():
    n_c = np.full(8, 2)
    out = rr.resolve(np.zeros((8, 2, 2, 3)), n_c)
    assert (out["j"] == 0).all() and (out["G"] == 0).all() and (out["image"] == 0).all()
    out = rr.resolve(np.ones((8, 2, 2, 3)), np.zeros(8, int))
    assert (out["j"] == 0).all() and (out["image"] == 0).all()
    # a NaN total counts as G = 0
    chains = _flat([1.0] * 8, n_c)
    chains[3, 0, 0, 1] = np.nan
    out = rr.resolve(chains, n_c)
    assert out["j"][0, 0] == 0 and out["G"][0, 0] == 0 and (out["j"] == 0).all()


# ---- rene_robust_combine ---------------------------------------------------------------------------------------------------------------
def _part(fig, n_frames=24, max_trim=3, gain=1.0):
    s = abi.RobustSummary()
    s.struct_size = C.sizeof(abi.RobustSummary)
    for k in ("n_tiles", "n_pixels", "n_trimmed", "sum_lum_plain", "sum_lum_robust", "kept_energy"):
        setattr(s, k, fig[k])
    s.n_frames, s.max_trim, s.gain = n_frames, max_trim, gain
    return s


def test_combine_of_parts_equals_the_whole(hip_lib):
    rng = np.random.default_rng(5)
    ty, tx = 5, 7  # a 200 x 150 image: ragged on both sides
    n = np.full((ty, tx), 1024)
    n[-1, :] = 22 * 32
    n[:, -1] = 8 * 32
    n[-1, -1] = 22 * 8
    a = (rng.uniform(0.0, 2.0, (ty, tx)) * n).astype(np.float32)
    b = (a * rng.uniform(0.5, 1.0, (ty, tx))).astype(np.float32)
    nt = (n * rng.uniform(0.0, 0.3, (ty, tx))).astype(np.int64)
    a[1, 2] = b[1, 2] = nt[1, 2] = 0  # a black tile
    whole = rr.summary(a, b, n, nt)
    for count in (2, 3, 8, 40):  # 40 shards of 35 tiles: five own none
        owner = np.arange(ty * tx).reshape(ty, tx) % count
        parts = [_part(rr.summary(a, b, n, nt, owned=owner == r), n_frames=24 if r else 16) for r in range(count)]
        got = api.robust_combine(parts)
        assert got.struct_size == 64 and got.n_frames == 24 and got.max_trim == 3 and got.gain == 1.0  # n_frames: the largest
        assert got.n_tiles == whole["n_tiles"] == ty * tx and got.n_pixels == whole["n_pixels"] == int(n.sum()) and got.n_trimmed == whole["n_trimmed"] == int(nt.sum())
        for k in ("sum_lum_plain", "sum_lum_robust", "kept_energy"):
            assert abs(getattr(got, k) - whole[k]) <= 1e-12 * abs(whole[k]), (count, k)
    one = api.robust_combine([_part(whole)])
    assert one.kept_energy == whole["sum_lum_robust"] / whole["sum_lum_plain"] and 0.5 < one.kept_energy < 1
    empty = abi.RobustSummary()
    empty.struct_size, empty.max_trim, empty.gain = 64, 3, 1.0
    assert api.robust_combine([empty]).kept_energy == 1.0  # nothing to keep: 1 by definition
    assert api.robust_combine([empty, _part(whole)]).kept_energy == one.kept_energy

    def code(parts):
        with pytest.raises(api.ReneError) as e:
            api.robust_combine(parts)
        assert str(e.value).split(": ", 1)[1].strip()
        return e.value.code

    assert code([_part(whole), _part(whole, max_trim=2)]) == -1
    assert code([_part(whole), _part(whole, gain=0.5)]) == -1
    bad = _part(whole)
    bad.struct_size = 56
    assert code([_part(whole), bad]) == -1
    assert code([]) == -1


# ---- the specification on oracle renders ------------------------------------------------------------------------------------------------
def _oracle_chains(o, spp, marks):
    """The chains of frames 0 .. m - 1 for every m in marks (ascending), default seed."""
    chains = np.zeros((8, o.yres, o.xres, 3), np.float32)
    out = {}
    for fr in range(spp):
        o.reset()
        o.render(fr, 1, threads=THREADS)
        chains[fr % 8] += o.download(0)
        if fr + 1 in marks:
            out[fr + 1] = chains.copy()
    return out


def _oracle_reference(o):
    o.reset()
    o.render(REF_FIRST, REF_FRAMES, threads=THREADS)
    return o.download(0).astype(np.float64) / REF_FRAMES


def _energy(img, ref):
    return float(np.mean(img) / np.mean(ref))


def test_robust_halves_the_error_on_veach_mis(oracle_mod):
    """veach_mis(96, 54) at 32 frames, default seed, against 1024 oracle frames from frame 100000: relMSE 2.21 -> 0.052 when the rule was
    written (ratio 0.024); the bound is the issue's 0.5."""
    o = oracle_mod.Oracle(scenes.veach_mis(96, 54))
    ref = _oracle_reference(o)
    chains = _oracle_chains(o, 32, (32,))[32]
    out = rr.resolve(chains, rr.chain_counts(32))
    e_plain, e_robust = relmse(out["plain"], ref), relmse(out["image"], ref)
    print(f"veach-mis @ 32: relMSE plain {e_plain:.4f}, robust {e_robust:.4f} (ratio {e_robust / e_plain:.4f}); energy plain {_energy(out['plain'], ref):.3f}, "
          f"robust {_energy(out['image'], ref):.3f}; trimmed pixels {float((out['j'] > 0).mean()):.3f}")
    assert e_robust <= 0.5 * e_plain, (e_robust, e_plain)


def test_robust_halves_the_error_on_fog_and_converges_to_the_mean(oracle_mod):
    """cornell_fog(64, 64), default seed: relMSE at 16 frames 0.15 of the plain mean's when the rule was written (bound: the issue's 0.5), and
    the energy kept at 64 frames is at least that at 16 (0.58 -> 0.70): the estimator converges to the mean."""
    o = oracle_mod.Oracle(scenes.cornell_fog(64, 64))
    ref = _oracle_reference(o)
    at = _oracle_chains(o, 64, (16, 64))
    kept = {}
    for spp in (16, 64):
        out = rr.resolve(at[spp], rr.chain_counts(spp))
        s = rr.summary(*rr.tile_records(out["lum_plain"], out["lum_robust"], out["j"]))
        kept[spp] = s["kept_energy"]
        e_plain, e_robust = relmse(out["plain"], ref), relmse(out["image"], ref)
        print(f"fog @ {spp}: relMSE plain {e_plain:.4f}, robust {e_robust:.4f} (ratio {e_robust / e_plain:.4f}); energy plain {_energy(out['plain'], ref):.3f}, "
              f"robust {_energy(out['image'], ref):.3f}; kept_energy {s['kept_energy']:.3f}; trimmed pixels {s['n_trimmed'] / s['n_pixels']:.3f}")
        if spp == 16:
            assert e_robust <= 0.5 * e_plain, (e_robust, e_plain)
    assert kept[64] >= kept[16], kept


# ---- the build -----------------------------------------------------------------------------------------------------------------------------
def test_unit_is_built_without_contraction_and_without_spills(hip_lib):
    """The Makefile builds kernels_robust.hip with the IEEE division, denormals and no fused multiply-add -- in the product and in `make variant`
    -- and the compiler's report (kernels_robust.res) shows no scratch and no spills."""
    import re
    mk = open(os.path.join(ROOT, "rene_amd", "csrc", "Makefile")).read()
    assert "kernels_robust.o" in mk.split("OBJS =")[1].splitlines()[0] and "2> kernels_robust.res" in mk
    flags = [l for l in mk.splitlines() if l.startswith("ROBUSTFLAGS")][0]
    assert "-ffp-contract=off" in flags and "$(MEANFLAGS)" in flags and "filter-out -ffp-contract=on" in flags
    assert "$(ROBUSTFLAGS) $(RESFLAGS) $(EXTRA) -c -o var_$(NAME)/kernels_robust.o" in mk
    text = open(os.path.join(ROOT, "rene_amd", "csrc", "kernels_robust.res")).read()
    ks = re.findall(r"Function Name: (\S+)", text)
    assert len(ks) == 1 and "robust_tiles_kernel" in ks[0], ks
    g = lambda key: int(re.search(re.escape(key) + r": (\d+)", text).group(1))
    assert g("ScratchSize [bytes/lane]") == 0 and g("SGPRs Spill") == 0 and g("VGPRs Spill") == 0
    assert 0 < g("LDS Size [bytes/block]") <= 256 and g("Occupancy [waves/SIMD]") >= 2
