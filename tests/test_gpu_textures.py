"""-m gpu: the texture unit and the environment look-up per sample against the fp64 reference of tests/texture_reference.py, whose allowance
comes from its own sensitivity (its module docstring); tests/test_texture_reference.py shows on the CPU that the oracle meets the same bounds
on the same inputs and that the inputs stay within their caps.

Surface textures go through rene_bsdf_eval: a Matte's only lobe holds tex_color(kd, uv), and with wo = wi = n its f is that colour times
fp32(1 / pi) -- one multiply, 2 ulp added to the allowance.  Every probe runs twice, on a context whose materials were resolved at upload
and on one under RENE_NO_RESOLVE, and the two answers are bit-identical.
- Image maps of 5 x 7 (RGB), 4 x 8 (RGBA), 1 x 1, 1 x 6, 6 x 1 and 64 x 64 texels, none at offset 0 of the image pool: 4 096 uniform uv in
  [-9, 9]^2 each, none left out; the seams (0, -0, 1, the floats next to 0 and 1, the first and last texel centre, crossed); coordinates with
  u W, v H at +- 2^23, 2^31, 2^35.
- The texel centres of the 4 x 8 image over the periods -1000, -3 .. 2, 999: texel x fp32(1 / pi) bit for bit, through the 1 - v flip, at
  texel indices either side of -n, 0, n and 2 n (the two paths of `wrap`).
- Checkerboards (of images, of solids, of a checkerboard -- which reads 1 --, with power-of-two scales): the uniform set within the
  allowance, and a lattice on which u su, v sv are exact in fp32, cell edges included, bit for bit against the oracle.
- Scales: image x image, image x solid, image x checkerboard (= image x 1, bit for bit the image).

The environment goes through one-frame renders of a 77 x 45 film: after reset(), render(f, 1) leaves background_color x look-up(d) in layer 0
of a missed pixel, d the device's own ray direction from primary_hits(f, 1); frames 0, 5 and 13.  The +z pole and the phi = 0 seam are in
view.  Kernels, each named by the launch log as kernel_matrix.expected_kernel restates: the BVH kernel on a scene without instances, the item
loop, the same scene forced onto the BVH and onto the wavefront integrator (which logs no megakernel), the restart kernel with its tables
in LDS and in global memory, the while-while kernel, and the volpath item loop and restart kernel.  Backgrounds: a random 16 x 8 image, one
whose pole rows are constant, the random one behind a non-uniform scale, a Solid, a Checkerboard of two images and a Scale; each bit-identical
under RENE_NO_RESOLVE (which takes an ImageMap or a Solid through the texture tables instead of Uniforms::bg_*).  render(0, 4) on the item
loop is held to four allowances plus the sum's roundings.

Largest error / allowance observed on an MI355X (a record, not a threshold; the oracle's own on the same inputs in brackets):
  image maps      uniform 0.50 (0.52), seams 0.07 (0.07); texel centres bit for bit; large coordinates bit for bit where the oracle is exact
  checkerboards   uniform 0.27 (0.27), lattice 0.27 against fp64 and bit for bit against the oracle
  scales          0.45 (0.45)
  environment     0.24 on the Checkerboard and 0.19 on an image, the same on the item loop, the BVH kernel with and without instances, the
                  wavefront integrator, the restart kernel (tables in LDS or global) and the while-while kernel (0.20 / 0.20); the volpath
                  item loop and restart kernel, whose camera looks elsewhere, 0.20 and 0.16 (0.97 on one sample at a cell edge / 0.44);
                  render(0, 4) 0.07
"""
import numpy as np
import pytest

import kernel_matrix as km
import texture_reference as tr
from rene_amd import abi, api

pytestmark = pytest.mark.gpu

S = tr.surface_scene()


@pytest.fixture(scope="module")
def contexts():
    """The surface scene on two contexts: materials resolved at upload, and under RENE_NO_RESOLVE (read when the scene is packed)."""
    mp = pytest.MonkeyPatch()
    mp.delenv("RENE_NO_RESOLVE", raising=False)
    resolved = api.Renderer(S.scene)
    mp.setenv("RENE_NO_RESOLVE", "1")
    tables = api.Renderer(S.scene)
    mp.undo()
    yield resolved, tables
    resolved.close()
    tables.close()


def _f(contexts, case, uv):
    """The device's f per sample, (n, 3): one lobe, and the same bits with and without the resolve."""
    uv = np.ascontiguousarray(uv, np.float32)
    n, wo, wi, seeds = tr.probe_inputs(len(uv))
    g = [r.bsdf_eval(S.material[case], n, uv, wo, wi, seeds) for r in contexts]
    assert (g[0][:, 11] == 1).all() and np.array_equal(g[0].view(np.uint32), g[1].view(np.uint32)), case
    return g[0][:, :3]


def _held(contexts, case, uv, what):
    tex = S.tex[case]
    got = _f(contexts, case, uv)
    ref, allow = tr.matte_f(S.scene, tex, uv[:, 0], uv[:, 1]), tr.matte_f_allowance(S.scene, tex, uv[:, 0], uv[:, 1])
    err = np.abs(got - ref)
    print(f"{case} {what}: {len(uv)} samples, error / allowance {tr.ratio(err, allow):.3f}")
    bad = (err > allow).any(-1) | ~np.isfinite(got).all(-1)
    assert not bad.any(), (case, what, int(bad.sum()), uv[bad][:4], got[bad][:4], ref[bad][:4])
    return got


# ---- surface textures -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tr.IMAGE_SHAPES)
def test_image_maps_on_the_uniform_set_and_the_seams(name, contexts):
    h, w = tr.IMAGE_SHAPES[name][:2]
    _held(contexts, "image-" + name, tr.uniform_uv("image-" + name), "uniform")
    _held(contexts, "image-" + name, tr.seam_uv(h, w), "seams")


def test_texel_centres_bit_for_bit(contexts):
    uv, row, col = tr.centre_uv()
    want = S.image["4x8"][row, col, :3] * tr.INV_PI32
    got = _f(contexts, "image-4x8", uv)
    bad = (got.view(np.uint32) != want.view(np.uint32)).any(-1)
    assert not bad.any(), (int(bad.sum()), uv[bad][:6], got[bad][:6], want[bad][:6])


@pytest.mark.parametrize("name", ("4x8", "5x7", "64x64", "1x6", "6x1"))
def test_large_coordinates_stay_inside_the_image(name, contexts, oracle_mod):
    """u W, v H at +- 2^23, 2^31, 2^35: past 2^24 a coordinate has no fraction left and the blend weights are 0 or 1/2, so every channel lies
    within the image's [min, max] exactly; where the oracle's look-up is the fp64 one (its coordinate arithmetic was exact) the device's is the
    oracle's bit for bit."""
    h, w = tr.IMAGE_SHAPES[name][:2]
    uv = tr.large_uv(h, w)
    got = _f(contexts, "image-" + name, uv)
    rgb = S.image[name][..., :3].reshape(-1, 3)
    assert np.isfinite(got).all() and (got >= rgb.min(0) * tr.INV_PI32).all() and (got <= rgb.max(0) * tr.INV_PI32).all()
    oracle = oracle_mod.Oracle(S.scene)
    agree = tr.oracle_agrees(oracle, S, name, uv)
    assert agree.any()
    assert np.array_equal(got[agree], tr.oracle_f(oracle, S.tex["image-" + name], uv)[agree]), uv[agree]


def test_a_solid_is_exact(contexts):
    got = _f(contexts, "solid", tr.uniform_uv("solid"))
    assert np.array_equal(got, np.broadcast_to(np.float32(tr.SOLID) * tr.INV_PI32, got.shape))


@pytest.mark.parametrize("case", tr.CHECKER_CASES)
def test_checkerboards_on_the_uniform_set(case, contexts):
    """(test_texture_reference.py: under 1 % of these samples have an allowance beyond 2 % of the children's contrast.)"""
    got = _held(contexts, case, tr.uniform_uv(case), "uniform")
    if case == "checker-of-checker":  # the Checkerboard child reads (1, 1, 1); the other is a Solid
        one = got == tr.INV_PI32
        assert 0.3 < one.all(-1).mean() < 0.7 and np.array_equal(got[~one.all(-1)], np.broadcast_to(np.float32([0.9, 0.1, 0.4]) * tr.INV_PI32, got[~one.all(-1)].shape))


@pytest.mark.parametrize("case", tr.CHECKER_CASES)
def test_checkerboard_lattice_matches_the_oracle_bit_for_bit(case, contexts, oracle_mod):
    uv = tr.lattice_uv()
    got = _held(contexts, case, uv, "lattice")
    want = tr.oracle_f(oracle_mod.Oracle(S.scene), S.tex[case], uv)
    bad = (got.view(np.uint32) != want.view(np.uint32)).any(-1)
    assert not bad.any(), (case, int(bad.sum()), uv[bad][:6], got[bad][:6], want[bad][:6])


@pytest.mark.parametrize("case", tr.SCALE_CASES)
def test_scales_on_the_uniform_set(case, contexts):
    uv = tr.uniform_uv(case)
    got = _held(contexts, case, uv, "uniform")
    if case == "scale-image-checker":  # image x (1, 1, 1)
        assert np.array_equal(got, _f(contexts, "image-5x7", uv))


# ---- the environment --------------------------------------------------------------------------------------------------------------------------------------
_B, _W, _R = abi.FLAG_FORCE_BVH, abi.FLAG_WAVEFRONT, abi.FLAG_NO_RESTART
KERNELS = {  # name -> geometry, context flags, RENE_NO_LDS_TABLES
    "bvh-no-instance": ("empty", 0, False), "item-loop": ("quad", 0, False), "bvh-forced": ("quad", _B, False), "wavefront": ("quad", _B | _W, False),
    "restart-lds-tables": ("room", 0, False), "restart-global-tables": ("room", 0, True), "while-while": ("room", _R, False),
    "volpath-item-loop": ("vol-room", 0, False), "volpath-restart": ("vol-deep", 0, False),
}


@pytest.fixture
def log(tmp_path, monkeypatch):
    path = str(tmp_path / "kernels.log")
    monkeypatch.setenv("RENE_TEST_KERNEL_LOG", path)
    return path


def _env(monkeypatch, name, value):
    if value:
        monkeypatch.setenv(name, "1")
    else:
        monkeypatch.delenv(name, raising=False)


def _primary_hits(scene, flags, frames):
    """The device's own rays and first hits per frame.  (The wavefront flag changes no ray: the probe runs on a context without it.)"""
    with api.Renderer(scene, flags=flags & ~_W) as r:
        return {f: r.primary_hits(f, 1)[0] for f in frames}


def _one_frame_renders(scene, flags, frames, log):
    km.read_log(log)
    with api.Renderer(scene, flags=flags) as r:
        out = {}
        for f in frames:
            r.reset()
            r.render(f, 1)
            out[f] = r.download(0)
    return out, [n for n in km.read_log(log) if "render_kernel" in n]


@pytest.mark.parametrize("background", tr.ENV_BACKGROUNDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_missed_pixels_hold_the_environment(kernel, background, log, monkeypatch):
    geometry, flags, no_lds_tables = KERNELS[kernel]
    s = tr.env_scene(geometry, background)
    want = km.expected_kernel(api.pack_info(s), flags, no_lds_tables)
    _env(monkeypatch, "RENE_NO_LDS_TABLES", no_lds_tables)
    images = {}
    for no_resolve in (False, True):
        _env(monkeypatch, "RENE_NO_RESOLVE", no_resolve)
        images[no_resolve], names = _one_frame_renders(s, flags, tr.ENV_FRAMES, log)
        assert names == ([] if flags & _W else [want] * len(tr.ENV_FRAMES)), (kernel, names, want)  # (the wavefront integrator launches no megakernel)
    _env(monkeypatch, "RENE_NO_RESOLVE", False)
    hits = _primary_hits(s, flags, tr.ENV_FRAMES)
    worst = 0.0
    for f in tr.ENV_FRAMES:
        got = images[False][f]
        assert np.array_equal(got.view(np.uint32), images[True][f].view(np.uint32)), (kernel, background, f, "RENE_NO_RESOLVE")
        miss = hits[f]["t"] < 0
        assert miss.mean() >= tr.MISS_SHARE
        d = hits[f]["d"][miss]
        ref, allow = tr.background(s, d), tr.background_allowance(s, d)[1]
        err = np.abs(got[miss] - ref)
        worst = max(worst, tr.ratio(err, allow))
        bad = (err > allow).any(-1) | ~np.isfinite(got[miss]).all(-1)
        assert not bad.any(), (kernel, background, f, int(bad.sum()), d[bad][:4], got[miss][bad][:4], ref[bad][:4])
        if background == "solid":
            assert np.array_equal(got[miss], np.broadcast_to(np.float32(tr.SOLID) * np.float32(tr.ENV_COLOR), got[miss].shape))
    print(f"{kernel} {background}: error / allowance {worst:.3f}")


def test_four_frames_sum_four_look_ups(log):
    """render(0, 4) on the item loop: a pixel all four of whose samples miss holds the sum of four terms -- four allowances, and (n - 1) ulp
    of the terms' magnitudes for a sum of n in any order."""
    s = tr.env_scene("quad", "random")
    got, names = _one_frame_renders(s, 0, (0,), log)  # (one frame, for the kernel's name)
    assert names == [km.expected_kernel(api.pack_info(s), 0)] and km.kernel_feat(names[0]) & km.SMALL
    with api.Renderer(s) as r:
        r.render(0, 4)
        got = r.download(0)
        hits = r.primary_hits(0, 4)
    miss = (hits["t"] < 0).all(0)
    assert miss.mean() >= tr.MISS_SHARE
    ref, allow, mag = 0.0, 0.0, 0.0
    for f in range(4):
        d = hits[f]["d"][miss]
        term = tr.background(s, d)
        ref, allow, mag = ref + term, allow + tr.background_allowance(s, d)[1], mag + np.abs(term)
    err = np.abs(got[miss] - ref)
    allow = allow + 3.0 * tr.EPS * mag
    print(f"render(0, 4): error / allowance {tr.ratio(err, allow):.3f}")
    assert (err <= allow).all(), int((err > allow).any(-1).sum())
