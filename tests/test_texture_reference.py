"""CPU: the fp64 texture and environment reference (tests/texture_reference.py) on values worked out by hand, against the oracle's fp32
restatement on every uv set and every environment scene the GPU tests use, and the caps those tests rely on -- shown here, on the oracle's
samples: how many samples a checkerboard or the environment sets aside, how many pixels miss, and that missed pixels lie at the seam and at
a pole."""
import numpy as np
import pytest

import texture_reference as tr
from rene_amd import abi

S = tr.surface_scene()


@pytest.fixture(scope="module")
def oracle(oracle_mod):
    return oracle_mod.Oracle(S.scene)


def _agrees(oracle, case, uv, what):
    tex = S.tex[case]
    ref, allow = tr.matte_f(S.scene, tex, uv[:, 0], uv[:, 1]), tr.matte_f_allowance(S.scene, tex, uv[:, 0], uv[:, 1])
    err = np.abs(tr.oracle_f(oracle, tex, uv) - ref)
    print(f"{case} {what}: oracle error / allowance {tr.ratio(err, allow):.3f}")
    assert (err <= allow).all(), (case, what, uv[(err > allow).any(-1)][:4])


# ---- the reference on values worked out by hand ---------------------------------------------------------------------------------------------------------
def test_image_sample_by_hand():
    img = np.arange(24, dtype=np.float64).reshape(2, 4, 3)  # h 2, w 4: texel (r, c) = 12 r + 3 c + channel
    at = lambda u, v: tr.image_sample(img, u, v)[..., 0]
    assert at(0.375, 0.25) == 3.0 and at(0.875, 0.75) == 21.0                    # centres of (0, 1) and (1, 3)
    assert at(1.0, 0.25) == at(0.0, 0.25) == at(-3.0, 0.25) == (9.0 + 0.0) / 2   # the seam: the last column with column 0
    assert at(0.375, 0.0) == at(0.375, 1.0) == (15.0 + 3.0) / 2                  # a pole: row h - 1 with row 0
    assert at(0.375 + 0.125, 0.25) == 4.5 and at(0.375 - 7.0, 0.25 + 5.0) == 3.0  # half way to the next texel; whole periods
    assert at(-0.125, 0.25) == 9.0 and at(-0.126, 0.25) < 9.0                     # floored modulo: texel -1 is texel w - 1
    assert tr.image_gradients(img) == (9.0, 12.0)                                  # the wrap included: |0 - 9|, |0 - 12|
    one = np.full((1, 1, 3), 0.25)
    assert (tr.image_sample(one, [-7.3, 0.0, 2.0 ** 40], [9.1, 1.0, -2.0 ** 33]) == 0.25).all() and tr.image_gradients(one) == (0.0, 0.0)


def test_kinds_by_hand():
    s, t = S.scene, S.tex
    img = S.image["4x8"]
    assert (tr.tex_color(s, t["solid"], 3.3, -8.0) == tr.SOLID).all()
    assert (tr.tex_color(s, t["image-4x8"], 1.5 / 8, 0.5 / 4) == img[3, 1, :3]).all()     # 1 - v: v = 1/8 is the LAST row
    other = np.float64(np.float32([0.9, 0.1, 0.4]))
    cs = lambda u, v: tr.tex_color(s, t["checker-solids"], u, v)                            # scales 2.5, 0.75
    assert (cs(0.2, 0.2) == tr.SOLID).all() and (cs(0.5, 0.2) == other).all() and (cs(0.5, 1.5) == tr.SOLID).all()
    assert (cs(-0.5, 0.2) == tr.SOLID).all() and (cs(-0.5, 1.5) == other).all()            # a negative coordinate truncates to 0
    assert (cs(2.0 ** 30, 0.2) == tr.SOLID).all() and (cs(2.0 ** 31, 0.2) == other).all()  # 5 * 2^29 is even; 5 * 2^30 saturates to 2^32 - 1, odd
    # checker-images: child 0 (4 x 8) where the parities agree, at fract -- not at (u, v)
    got = tr.tex_color(s, t["checker-images"], (1.0 + 1.5 / 8) / 6.0, (1.0 + 0.5 / 4) / 4.0)
    np.testing.assert_allclose(got, img[3, 1, :3], rtol=1e-12)
    # non-recursive: a Checkerboard child reads 1 -- in a checkerboard (scales 3, 5) and in a scale
    assert (tr.tex_color(s, t["checker-of-checker"], 0.1, 0.1) == 1.0).all() and (tr.tex_color(s, t["checker-of-checker"], 0.4, 0.1) == other).all()
    uv = tr.uniform_uv("scale-image-checker")
    assert (tr.tex_color(s, t["scale-image-checker"], uv[:, 0], uv[:, 1]) == tr.tex_color(s, t["image-5x7"], uv[:, 0], uv[:, 1])).all()
    a, b = (tr.tex_color(s, t[k], 0.3, 0.6) for k in ("image-5x7", "image-4x8"))
    assert (tr.tex_color(s, t["scale-image-image"], 0.3, 0.6) == a * b).all()


def test_parity_saturates():
    x = np.float64([-3.0, -0.0, 0.0, 0.99, 1.0, 2.5, 3.0, 2.0 ** 31, 2.0 ** 31 + 1, 2.0 ** 32 - 1, 2.0 ** 32, 2.0 ** 40])
    assert list(tr._parity(x)) == [0, 0, 0, 0, 1, 0, 1, 0, 1, 1, 1, 1]


def test_sphere_uv_by_hand():
    u, v = tr.sphere_uv(np.float64([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, -1e-300, 0]]))
    np.testing.assert_allclose(u, [0, 0.25, 0.5, 0.75, 0, 0, 1.0], atol=1e-15)  # (the last: just below the seam, phi + 2 pi)
    np.testing.assert_allclose(v, [0.5, 0.5, 0.5, 0.5, 1.0, 0.0, 0.5], atol=1e-15)
    s = tr.env_scene("empty", "random-nonuniform")
    m = np.asarray(s.background_matrix, np.float64)[:3, :3]
    d = np.float32([0.3, -0.5, 0.81])
    q = m @ d.astype(np.float64)
    np.testing.assert_allclose(tr.background_direction(s, d), q / np.sqrt(q @ q), rtol=1e-15)
    assert not np.allclose(m @ m.T, np.eye(3), atol=1e-3)  # a non-uniform scale: not a rotation
    r = np.asarray(tr.env_scene("empty", "random").background_matrix, np.float64)[:3, :3]
    assert np.allclose(r @ r.T, np.eye(3), atol=1e-6)


# ---- the oracle on the uv sets of the GPU tests ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tr.CASES)
def test_the_oracle_agrees_on_the_uniform_set(case, oracle):
    _agrees(oracle, case, tr.uniform_uv(case), "uniform")


@pytest.mark.parametrize("name", tr.IMAGE_SHAPES)
def test_the_oracle_agrees_on_the_seams(name, oracle):
    h, w = tr.IMAGE_SHAPES[name][:2]
    _agrees(oracle, "image-" + name, tr.seam_uv(h, w), "seams")


def test_texel_centres_read_the_texel_in_the_reference_and_in_the_oracle(oracle):
    """ax = ay = 0 at an exact texel centre: the fp64 reference returns the texel, the oracle texel x fp32(1 / pi) bit for bit -- through the
    1 - v flip and over every period, both sides of +- n and 2 n."""
    uv, row, col = tr.centre_uv()
    texel = S.image["4x8"][row, col, :3]
    assert (tr.tex_color(S.scene, S.tex["image-4x8"], uv[:, 0], uv[:, 1]) == texel).all()
    assert np.array_equal(tr.oracle_f(oracle, S.tex["image-4x8"], uv), texel * tr.INV_PI32)
    x = np.floor(uv[:, 0].astype(np.float64) * 8 - 0.5).astype(int)
    y = np.floor((1.0 - uv[:, 1].astype(np.float64)) * 4 - 0.5).astype(int)
    assert {-9, -8, -1, 0, 7, 8, 15, 16} <= set(x) and {-5, -4, -1, 0, 3, 4, 7, 8} <= set(y) and x.min() < -1000 and y.max() > 1000


@pytest.mark.parametrize("case", tr.CHECKER_CASES)
def test_the_lattice_is_exact_in_fp32_and_the_oracle_agrees(case, oracle):
    uv = tr.lattice_uv()
    t = S.scene.textures[S.tex[case]]
    for k in (0, 1):
        exact = uv[:, k].astype(np.float64) * float(t.v0[k])
        assert ((uv[:, k] * np.float32(t.v0[k])).astype(np.float64) == exact).all()
        assert (exact[exact > 0] == np.floor(exact[exact > 0])).sum() >= 81 * 2, "cell edges are on the lattice"
    _agrees(oracle, case, uv, "lattice")


@pytest.mark.parametrize("name", ("4x8", "5x7", "64x64", "1x6", "6x1"))
def test_large_coordinates_in_the_reference(name, oracle):
    """Indices modulo the size hold at 2^35 in fp64; the oracle's (int) cast does not, which is why the GPU test compares with it only where
    it agrees with fp64 to the blend's roundings (where its coordinate arithmetic was exact)."""
    h, w = tr.IMAGE_SHAPES[name][:2]
    uv = tr.large_uv(h, w)
    img = S.image[name]
    ref = tr.tex_color(S.scene, S.tex["image-" + name], uv[:, 0], uv[:, 1])
    assert np.isfinite(ref).all() and (ref >= img[..., :3].min((0, 1))).all() and (ref <= img[..., :3].max((0, 1))).all()
    agree = tr.oracle_agrees(oracle, S, name, uv)
    print(f"{name}: the oracle agrees with fp64 on {int(agree.sum())} of {len(uv)} large coordinates")
    assert agree.any()


def test_checkerboards_set_few_samples_aside():
    for case in tr.CHECKER_CASES:
        uv = tr.uniform_uv(case)
        share = (tr.tex_allowance(S.scene, S.tex[case], uv[:, 0], uv[:, 1]) > tr.SET_ASIDE * tr.tex_contrast(S.scene, S.tex[case])).mean()
        print(f"{case}: contrast {tr.tex_contrast(S.scene, S.tex[case]):.3f}, set aside {share:.4%}")
        assert share < tr.SET_ASIDE_CAP


def test_image_allowance_is_small_against_a_wrong_texel():
    for name in ("5x7", "4x8", "64x64"):
        uv = tr.uniform_uv("image-" + name)
        a = tr.tex_allowance(S.scene, S.tex["image-" + name], uv[:, 0], uv[:, 1])
        assert a.max() < 5e-4 * tr.image_contrast(S.image[name]) and np.median(a) < 1e-4 * tr.image_contrast(S.image[name]) and tr.image_contrast(S.image[name]) > 0.8


def test_a_matte_f_is_one_multiply(oracle):
    """oracle.bsdf_eval's f of a Matte with wo = wi = n is its tex_color times fp32(1 / pi), bit for bit."""
    n = np.float32([0, 0, 1])
    for case in ("image-5x7", "checker-images", "scale-image-image", "solid"):
        for uv in tr.uniform_uv(case)[:16]:
            e = oracle.bsdf_eval(S.material[case], n, uv, n, n)
            assert e["len"] == 1 and np.array_equal(e["f"], oracle.tex_color(S.tex[case], float(uv[0]), float(uv[1])) * tr.INV_PI32)


def test_the_images_under_test_do_not_start_the_pool():
    assert len(S.scene.images) == 3 + len(tr.IMAGE_SHAPES) and [im.shape[:2] for im in S.scene.images[3:]] == [v[:2] for v in tr.IMAGE_SHAPES.values()]
    for bg in ("random", "poles", "checker", "scale"):
        s = tr.env_scene("empty", bg)
        t = s.textures[s.background_texture]
        assert t.type == {"random": abi.TEXTURE_IMAGEMAP, "poles": abi.TEXTURE_IMAGEMAP, "checker": abi.TEXTURE_CHECKERBOARD, "scale": abi.TEXTURE_SCALE}[bg]
        first = t.u0[0] if t.type == abi.TEXTURE_IMAGEMAP else s.textures[t.u0[0]].u0[0]
        assert first >= 3


# ---- the environment scenes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", tr.ENV_GEOMETRY)
def test_environment_inputs_stay_within_their_caps(geometry):
    rays = tr.env_rays(geometry)
    d = np.concatenate([rays[f]["d"][rays[f]["t"] < 0] for f in tr.ENV_FRAMES])
    for f in tr.ENV_FRAMES:
        assert (rays[f]["t"] < 0).mean() >= tr.MISS_SHARE, (geometry, f)
    for bg in ("random", "random-nonuniform", "poles"):
        s = tr.env_scene(geometry, bg)
        u, v = tr.sphere_uv(tr.background_direction(s, d))
        x, y = u * 16, (1.0 - v) * 8
        assert (x < 1).any() and (x > 15).any() and (y < 1).any(), "missed pixels within one texel of either side of the seam and of the +z pole"
        aside = tr.background_allowance(s, d)[0] > tr.SET_ASIDE * tr.tex_contrast(s, s.background_texture)
        print(f"{geometry} {bg}: {len(d)} missed samples, {int((x < 1).sum() + (x > 15).sum())} at the seam, {int((y < 1).sum())} at the pole, set aside {int(aside.sum())}")
        assert aside.mean() <= (0.0 if bg == "poles" else tr.SET_ASIDE_CAP)


@pytest.mark.parametrize("background", tr.ENV_BACKGROUNDS)
@pytest.mark.parametrize("geometry", tr.ENV_GEOMETRY)
def test_the_oracle_miss_radiance_agrees(geometry, background, oracle_mod):
    s = tr.env_scene(geometry, background)
    o = oracle_mod.Oracle(s)
    rays = tr.env_rays(geometry)
    worst = 0.0
    for f in tr.ENV_FRAMES:
        o.reset()
        o.render(f, 1)
        miss = rays[f]["t"] < 0
        got, d = o.download(0)[miss], rays[f]["d"][miss]
        err, allow = np.abs(got - tr.background(s, d)), tr.background_allowance(s, d)[1]
        worst = max(worst, tr.ratio(err, allow))
        assert (err <= allow).all(), (f, int((err > allow).any(-1).sum()))
        if background == "solid":
            assert np.array_equal(got, np.broadcast_to(np.float32(tr.SOLID) * np.float32(tr.ENV_COLOR), got.shape))
    print(f"{geometry} {background}: oracle error / allowance {worst:.3f}")
