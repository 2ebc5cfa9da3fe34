"""Test helper (not a conftest): the texture unit and the environment look-up in numpy and float64, written from the specification -- the
comments above image_sample_at / tex_color / background_tex / sphere_uv in rene_amd/csrc/device_code.inc and the reference's texture.rs and
math.rs -- and not from the kernel's arithmetic.  Inputs (uv, the ray direction, the fp32 entries of background_matrix, texels) are taken as
exact; everything else is float64.

  image_sample(img, u, v)      bilinear, REPEAT: x = u W - 1/2, y = v H - 1/2, indices modulo the size (floored), the neighbour of the last
                               texel is texel 0
  tex_color(scene, tex, u, v)  Solid; ImageMap at (u, 1 - v); Checkerboard: the child by the parity of trunc(u su), trunc(v sv) (saturating: 0
                               for negatives, 2^32 - 1 above), looked up NON-recursively at fract; Scale: the product of two non-recursive
                               children.  Non-recursive: a Checkerboard or Scale child reads (1, 1, 1).
  sphere_uv(p), background(scene, d)
                               M d as a vector, normalized, theta = acos z, phi = atan2(y, x) (+ 2 pi where negative), u = phi / 2 pi,
                               v = (pi - theta) / pi, the background texture there, times background_color.  At a pole v is 0 or 1 and the
                               REPEAT look-up blends row 0 with row H - 1: that is the reference's sampler, and it is kept.

The allowance -- how far an fp32 evaluation of the same specification may be from this one -- comes from this reference's own sensitivity
and never from a device's output:

  image look-up   Gx ex + Gy ey + 8 2^-24 max|texel|.  Gx, Gy: the largest per-channel difference between adjacent texels along each axis,
                  the wrap included.  ex = 2^-23 (|u| W + 1/2), ey = 2^-23 (|1 - v| H + 1/2) + 2^-24 H max(1, |v|): the roundings of the three
                  fp32 operations that form x and y (1 - v; the multiply; the subtraction), times the slope of a piecewise-linear function.
                  The last term is the blend's roundings (1 - a, two products and a sum, twice).
  checkerboard    the largest change of the fp64 result with u su, v sv moved by +- 2 ulp (fp32, all eight combinations), plus the image term
                  of the children at the fract coordinates
  scale           a0 |c1| + a1 |c0| + a0 a1 + 2^-24 |c0 c1|
  environment     the largest change of the fp64 result with the components of the unit direction moved by +- BUDGET 2^-24 (all 26
                  combinations) or u, v moved by +- BUDGET 2^-24 (all 8), plus the texture's own term above at (u, v); times |background_color|,
                  plus 2 ulp for that multiply

BUDGET = 8 covers the matrix product (three products, two sums), the normalize (a dot product, an rsq, a multiply), and acosf / atan2f with
the two multiplies behind them.  No statement of the device library's ulp bounds for acosf and atan2f was found in the ROCm installation
(its documentation and headers were searched), so the 8 is ASSUMED, not measured: the OpenCL C bounds for the same functions in full
profile are 4 and 6 ulp of a result whose magnitude is at most pi.

For scale: a wrong texel, row, flip or seam is an error of the order of G (about 0.9 for a random image of 64 texels and more); the allowance
of a well-conditioned sample is about 1e-5 G.

The second half holds the inputs the CPU and the GPU tests share: one scene of Matte materials over every texture kind (a Matte's only lobe
is tex_color(kd, uv), so rene_bsdf_eval's f with wo, wi on the normal's side is that colour times fp32(1 / pi)), its uv sets, and the
environment scenes."""
import itertools

import numpy as np

from rene_amd import abi, glam
from rene_amd.scene import Scene, TriangleMesh

EPS = 2.0 ** -24
BUDGET = 8.0
INV_PI32 = np.float32(0.318309886183790671538)  # the Lambert lobe's constant (bxdf.rs:87-89)
SET_ASIDE = 0.02  # a sample whose allowance exceeds this share of the contrast (G of an image, the children's contrast of a checkerboard) says little
SET_ASIDE_CAP = 0.01


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------------
def _rgb(img):
    return np.asarray(img, np.float64)[..., :3]


def _uv(u, v):
    return np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(v, np.float64))


def image_sample(img, u, v):
    t = _rgb(img)
    H, W = t.shape[:2]
    u, v = _uv(u, v)
    x, y = u * W - 0.5, v * H - 0.5
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = (x - fx)[..., None], (y - fy)[..., None]
    x0, y0 = fx.astype(np.int64) % W, fy.astype(np.int64) % H  # floored: -1 % W == W - 1
    x1, y1 = (x0 + 1) % W, (y0 + 1) % H
    top = t[y0, x0] * (1.0 - ax) + t[y0, x1] * ax
    bottom = t[y1, x0] * (1.0 - ax) + t[y1, x1] * ax
    return top * (1.0 - ay) + bottom * ay


def image_gradients(img):
    """(Gx, Gy): the largest per-channel difference between adjacent texels along u and along v, the wrap included."""
    t = _rgb(img)
    return float(np.abs(t - np.roll(t, -1, axis=1)).max()), float(np.abs(t - np.roll(t, -1, axis=0)).max())


def image_contrast(img):
    return max(image_gradients(img))


def image_blend_term(img):
    return 8.0 * EPS * float(np.abs(_rgb(img)).max())


def image_allowance(img, u, v):
    """Of an ImageMap texture at the texture's (u, v): the look-up is at (u, 1 - v)."""
    H, W = np.asarray(img).shape[:2]
    u, v = _uv(u, v)
    gx, gy = image_gradients(img)
    ex = 2.0 * EPS * (np.abs(u) * W + 0.5)
    ey = 2.0 * EPS * (np.abs(1.0 - v) * H + 0.5) + EPS * H * np.maximum(1.0, np.abs(v))
    return gx * ex + gy * ey + image_blend_term(img)


def _solid(t, shape):
    return np.broadcast_to(np.float64([t.v0[0], t.v0[1], t.v0[2]]), shape + (3,)).copy()


def _non_recursive(scene, tex, u, v):
    t = scene.textures[tex]
    if t.type == abi.TEXTURE_SOLID:
        return _solid(t, u.shape)
    if t.type == abi.TEXTURE_IMAGEMAP:
        return image_sample(scene.images[t.u0[0]], u, 1.0 - v)
    return np.ones(u.shape + (3,))


def _non_recursive_allowance(scene, tex, u, v):
    t = scene.textures[tex]
    if t.type == abi.TEXTURE_IMAGEMAP:
        return image_allowance(scene.images[t.u0[0]], u, v)
    return np.zeros(u.shape)


def _parity(x):
    """f32_to_u32(x) % 2: truncation, 0 for negatives (and -0), 2^32 - 1 from 2^32 on."""
    return np.where(x > 0, np.floor(np.minimum(x, 4294967295.0)), 0.0) % 2


def _checker(scene, t, x, y):
    same = _parity(x) == _parity(y)
    fu, fv = x - np.floor(x), y - np.floor(y)
    return np.where(same[..., None], _non_recursive(scene, t.u0[0], fu, fv), _non_recursive(scene, t.u0[1], fu, fv))


def tex_color(scene, tex, u, v):
    t = scene.textures[tex]
    u, v = _uv(u, v)
    if t.type == abi.TEXTURE_CHECKERBOARD:
        return _checker(scene, t, u * float(t.v0[0]), v * float(t.v0[1]))
    if t.type == abi.TEXTURE_SCALE:
        return _non_recursive(scene, t.u0[0], u, v) * _non_recursive(scene, t.u0[1], u, v)
    return _non_recursive(scene, tex, u, v)


def _ulp32(x):
    with np.errstate(over="ignore"):
        return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def tex_allowance(scene, tex, u, v):
    """Per sample (one number for the three channels)."""
    t = scene.textures[tex]
    u, v = _uv(u, v)
    if t.type == abi.TEXTURE_CHECKERBOARD:
        x, y = u * float(t.v0[0]), v * float(t.v0[1])
        base = _checker(scene, t, x, y)
        worst = np.zeros(u.shape)
        for sx, sy in itertools.product((-2.0, 0.0, 2.0), repeat=2):
            if sx or sy:
                worst = np.maximum(worst, np.abs(_checker(scene, t, x + sx * _ulp32(x), y + sy * _ulp32(y)) - base).max(-1))
        fu, fv = x - np.floor(x), y - np.floor(y)
        return worst + np.maximum(_non_recursive_allowance(scene, t.u0[0], fu, fv), _non_recursive_allowance(scene, t.u0[1], fu, fv))
    if t.type == abi.TEXTURE_SCALE:
        a0, a1 = (_non_recursive_allowance(scene, t.u0[k], u, v) for k in (0, 1))
        c0, c1 = (_non_recursive(scene, t.u0[k], u, v) for k in (0, 1))
        return a0 * np.abs(c1).max(-1) + a1 * np.abs(c0).max(-1) + a0 * a1 + EPS * np.abs(c0 * c1).max(-1)
    return _non_recursive_allowance(scene, tex, u, v)


def tex_contrast(scene, tex):
    """What a wrong look-up moves the colour by, to the order of magnitude: G of an image; for a checkerboard the largest distance between
    a value of one child and a value of the other."""
    t = scene.textures[tex]

    def span(k):
        c = scene.textures[k]
        if c.type == abi.TEXTURE_SOLID:
            s = np.float64([c.v0[0], c.v0[1], c.v0[2]])
            return s, s
        if c.type == abi.TEXTURE_IMAGEMAP:
            rgb = _rgb(scene.images[c.u0[0]]).reshape(-1, 3)
            return rgb.min(0), rgb.max(0)
        return np.ones(3), np.ones(3)

    if t.type == abi.TEXTURE_IMAGEMAP:
        return image_contrast(scene.images[t.u0[0]])
    if t.type == abi.TEXTURE_CHECKERBOARD:
        (lo0, hi0), (lo1, hi1) = span(t.u0[0]), span(t.u0[1])
        return float(np.maximum(hi0 - lo1, hi1 - lo0).max())
    raise ValueError("an ImageMap or a Checkerboard")


def matte_f(scene, tex, u, v):
    """f of a Matte over `tex` with wo, wi on the normal's side: one multiply by fp32(1 / pi)."""
    return tex_color(scene, tex, u, v) * float(INV_PI32)


def matte_f_allowance(scene, tex, u, v):
    """(n, 3): the colour's allowance through the multiply, and the multiply's rounding (2 ulp)."""
    return tex_allowance(scene, tex, u, v)[..., None] * float(INV_PI32) + 2.0 * EPS * np.abs(matte_f(scene, tex, u, v))


def sphere_uv(p):
    p = np.asarray(p, np.float64)
    theta = np.arccos(np.clip(p[..., 2], -1.0, 1.0))
    phi = np.arctan2(p[..., 1], p[..., 0])
    phi = np.where(phi < 0, phi + 2.0 * np.pi, phi)
    return phi / (2.0 * np.pi), (np.pi - theta) / np.pi


def background_direction(scene, d):
    """normalize(M d), M the upper 3 x 3 of the fp32 background_matrix, d the fp32 ray direction -- both exact inputs."""
    m = np.asarray(scene.background_matrix, np.float32).astype(np.float64)[:3, :3]
    q = np.asarray(d, np.float32).astype(np.float64) @ m.T
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _background_color(scene):
    return np.float32(scene.background_color).astype(np.float64)


def background(scene, d):
    u, v = sphere_uv(background_direction(scene, d))
    return tex_color(scene, scene.background_texture, u, v) * _background_color(scene)


def background_allowance(scene, d):
    """(texture, radiance): the allowance of the looked-up colour, one number per sample, and of the radiance, per channel."""
    tex = scene.background_texture
    p = background_direction(scene, d)
    u, v = sphere_uv(p)
    base = tex_color(scene, tex, u, v)
    delta = BUDGET * EPS
    worst = np.zeros(u.shape)
    for s in itertools.product((-1.0, 0.0, 1.0), repeat=3):
        if any(s):
            worst = np.maximum(worst, np.abs(tex_color(scene, tex, *sphere_uv(p + delta * np.float64(s))) - base).max(-1))
    for su, sv in itertools.product((-1.0, 0.0, 1.0), repeat=2):
        if su or sv:
            worst = np.maximum(worst, np.abs(tex_color(scene, tex, u + delta * su, v + delta * sv) - base).max(-1))
    worst = worst + tex_allowance(scene, tex, u, v)
    c = _background_color(scene)
    return worst, worst[..., None] * np.abs(c) + 2.0 * EPS * np.abs(base * c)


def ratio(err, allowance):
    """The largest error / allowance; an error of 0 counts 0 whatever the allowance (a Solid's is 0)."""
    err, allowance = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(allowance, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / allowance)
    return float(r.max()) if r.size else 0.0


# ---- surface textures: one scene, its cases and its uv sets ------------------------------------------------------------------------------------------
IMAGE_SHAPES = {"5x7": (5, 7, 3), "4x8": (4, 8, 4), "1x1": (1, 1, 3), "1x6": (1, 6, 3), "6x1": (6, 1, 3), "64x64": (64, 64, 3)}  # h, w, channels
IMAGE_CASES = tuple("image-" + k for k in IMAGE_SHAPES)
CHECKER_CASES = ("checker-images", "checker-solids", "checker-of-checker", "checker-pow2")
SCALE_CASES = ("scale-image-image", "scale-image-solid", "scale-image-checker")
CASES = IMAGE_CASES + ("solid",) + CHECKER_CASES + SCALE_CASES
SOLID = (0.25, 0.5, 0.75)
N_UNIFORM = 4096
PERIODS = (-1000, -3, -2, -1, 0, 1, 2, 999)


class Surface:
    """scene, tex[case] (texture index), material[case], image[name] (the (h, w, 4) array the scene holds)."""


def _filler_images(s, rng):
    for h, w in ((3, 3), (2, 5), (7, 2)):  # three images ahead of every image under test: none sits at offset 0 of the pool
        s.add_texture_image_map(rng.random((h, w, 3), dtype=np.float32))


def surface_scene() -> Surface:
    rng = np.random.default_rng(20240)
    s = Scene.new()
    s.set_camera(glam.look_at_lh((0.0, 0.0, -4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), 40.0, 16, 16)
    _filler_images(s, rng)
    out = Surface()
    out.scene, out.tex, out.material, out.image = s, {}, {}, {}
    for name, shape in IMAGE_SHAPES.items():
        out.tex["image-" + name] = s.add_texture_image_map(rng.random(shape, dtype=np.float32))
        out.image[name] = s.images[-1]
    t = out.tex
    t["solid"] = s.add_texture_solid(SOLID)
    other = s.add_texture_solid((0.9, 0.1, 0.4))
    t["checker-images"] = s.add_texture_checkerboard(t["image-4x8"], t["image-64x64"], 6.0, 4.0)
    t["checker-solids"] = s.add_texture_checkerboard(t["solid"], other, 2.5, 0.75)
    t["checker-of-checker"] = s.add_texture_checkerboard(t["checker-solids"], other, 3.0, 5.0)  # the first child reads (1, 1, 1)
    t["checker-pow2"] = s.add_texture_checkerboard(t["image-64x64"], t["image-4x8"], 4.0, 2.0)
    t["scale-image-image"] = s.add_texture_scale(t["image-5x7"], t["image-4x8"])
    t["scale-image-solid"] = s.add_texture_scale(t["image-5x7"], t["solid"])
    t["scale-image-checker"] = s.add_texture_scale(t["image-5x7"], t["checker-solids"])  # image x (1, 1, 1)
    tri = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    for k, case in enumerate(CASES):  # an instance per material: the probe then runs on the record a render would use (Inst::res_*)
        out.material[case] = s.add_matte(t[case])
        s.add_triangle_mesh(TriangleMesh.from_arrays(tri + np.float32([2.0 * k - 13.0, 0, 0]), np.uint32([0, 1, 2])), out.material[case])
    return out


def uniform_uv(case):
    return np.random.default_rng(1000 + CASES.index(case)).uniform(-9.0, 9.0, (N_UNIFORM, 2)).astype(np.float32)


def centre_uv():
    """The texel centres of the 4 x 8 image over the periods k, m: u = k + (j + 1/2) / 8, v = m + (i + 1/2) / 4, exact in fp32.  Returns the
    uv (n, 2) and the texel (row, column) each must read: column j, row 3 - i (the 1 - v flip)."""
    k, m, j, i = (a.reshape(-1) for a in np.meshgrid(PERIODS, PERIODS, np.arange(8), np.arange(4), indexing="ij"))
    u, v = k + (j + 0.5) / 8.0, m + (i + 0.5) / 4.0
    uv = np.stack([u, v], -1).astype(np.float32)
    assert (uv.astype(np.float64) == np.stack([u, v], -1)).all()
    return uv, 3 - i, j


def seam_uv(h, w):
    one, zero = np.float32(1), np.float32(0)

    def axis(n):
        return np.float32([0.0, -0.0, 1.0, np.nextafter(one, zero), np.nextafter(zero, -one), 0.5 / n, 1.0 - 0.5 / n])
    return np.array(list(itertools.product(axis(w), axis(h))), np.float32)


def large_uv(h, w):
    """u W and v H at +- 2^23, +- 2^31, +- 2^35 -- beyond the (int) cast -- each axis against a moderate other and against itself."""
    big = [s * 2.0 ** e for e in (23, 31, 35) for s in (1, -1)]
    us, vs = [b / w for b in big] + [0.3, -2.7], [b / h for b in big] + [0.6, -1.1]
    return np.array(list(itertools.product(us, vs)), np.float32)


def lattice_uv():
    """Multiples of 1/8 in [-2, 8]: with the scales of every checkerboard here (6, 4, 2.5, 0.75, 3, 5, 2) u su and v sv are exact in fp32, and
    cell edges are among them (u = 1/2 under 6, every multiple of 1/4 under 4, u = 2, 4 under 2.5, v = 4 under 0.75).  The fract coordinates
    are multiples of 1/8: in the 4 x 8 and 64 x 64 children the blend weights are then 0 or 1/2 and every product is exact, so contracted
    and uncontracted fp32 evaluations of the blend agree bit for bit."""
    a = np.arange(-16, 65) / 8.0
    return np.array(list(itertools.product(a, a)), np.float32)


def probe_inputs(n):
    """normals, wo, wi for the probe: all +z, so that f is the lobe's colour times fp32(1 / pi)."""
    z = np.zeros((n, 3), np.float32)
    z[:, 2] = 1
    return z, z.copy(), z.copy(), np.zeros(n, np.uint32)


def oracle_f(oracle, tex, uv):
    """Oracle.tex_color per sample times fp32(1 / pi), in fp32: what the device's f must be where both evaluate the same fp32 expression."""
    c = np.array([oracle.tex_color(tex, float(u), float(v)) for u, v in uv], np.float32).reshape(-1, 3)
    return c * INV_PI32


def oracle_agrees(oracle, surface, name, uv):
    """Where the oracle's look-up into image `name` is the fp64 one to the blend's roundings: its coordinate arithmetic was exact there."""
    tex = surface.tex["image-" + name]
    got = np.array([oracle.tex_color(tex, float(u), float(v)) for u, v in uv], np.float64).reshape(-1, 3)
    return (np.abs(got - tex_color(surface.scene, tex, uv[:, 0], uv[:, 1])) <= image_blend_term(surface.image[name])).all(-1)


# ---- the environment: scenes of one 77 x 45 frame whose missed pixels hold background_color x look-up(d) --------------------------------------------
ENV_FRAMES = (0, 5, 13)
ENV_COLOR = (0.5, 1.0, 2.0)
# no instance (a scene without instances is not packed for the item loop); one quad (the item loop); the kernel matrix's room with its deep mesh
# and the background its only light (the restart and while-while kernels); its volpath rooms, shallow and deep, the camera outside the media
ENV_GEOMETRY = ("empty", "quad", "room", "vol-room", "vol-deep")
ENV_BACKGROUNDS = ("random", "poles", "random-nonuniform", "solid", "checker", "scale")
MISS_SHARE = 0.6


ENV_EYE = (0.0, 1.0, -5.0)
ENV_TARGET_Y = {"empty": 3.0, "quad": 3.0, "room": 3.0, "vol-room": 4.5, "vol-deep": 4.5}  # the room fills the film's lower fifth, the fog's boundary its lower third


def _env_ctm(nonuniform, target_y):
    """A rotation that puts the +z pole a few degrees off the view's centre and with it the phi = 0 seam, a meridian that leaves the pole,
    into the view; `nonuniform` scales the map's axes behind it."""
    view = np.float64([0.0, target_y, 0.0]) - np.float64(ENV_EYE)
    view /= np.linalg.norm(view)
    pole = view + np.float64([0.12, 0.05, 0.0])
    pole /= np.linalg.norm(pole)
    axis = np.cross([0.0, 0.0, 1.0], pole)
    r = glam.mul(glam.from_axis_angle(axis / np.linalg.norm(axis), float(np.arccos(pole[2]))), glam.from_axis_angle((0.0, 0.0, 1.0), 0.7))
    return glam.mul(r, glam.from_scale((1.0, 0.8, 1.25))) if nonuniform else r


def env_images():
    rng = np.random.default_rng(77)
    random = rng.random((8, 16, 3), dtype=np.float32)
    poles = rng.random((8, 16, 3), dtype=np.float32)
    poles[0], poles[7] = poles[0, 0].copy(), poles[7, 0].copy()  # rows 0 and 7 constant along u: tight at the poles whatever phi is
    return random, poles, rng.random((8, 16, 3), dtype=np.float32)


def env_scene(geometry, background):
    import kernel_matrix as km
    if geometry == "empty":
        s = Scene.new()
    elif geometry == "quad":  # the room's back wall alone
        s = Scene.new()
        s.add_triangle_mesh(km._quad([[-2.5, 0, 2.5], [-2.5, 2.5, 2.5], [2.5, 2.5, 2.5], [2.5, 0, 2.5]]), s.add_matte((0.5, 0.3, 0.25)))
    else:
        s = {"room": lambda: km.room(deep="matte", emitter=None),  # the background is its only light
             "vol-room": lambda: km.room(volpath=True, sun=True), "vol-deep": lambda: km.room(deep="matte", volpath=True, sun=True)}[geometry]()
    s.set_camera(glam.look_at_lh(ENV_EYE, (0.0, ENV_TARGET_Y[geometry], 0.0), (0.0, 1.0, 0.0)), 38.0, km.W, km.H)
    _filler_images(s, np.random.default_rng(78))
    random, poles, third = env_images()
    s.background_color = ENV_COLOR
    s.background_matrix = glam.inverse(_env_ctm(background == "random-nonuniform", ENV_TARGET_Y[geometry]))
    if background == "solid":
        s.background_texture = s.add_texture_solid(SOLID)
    elif background == "poles":
        s.background_texture = s.add_texture_image_map(poles)
    else:
        s.background_texture = a = s.add_texture_image_map(random)
        if background == "checker":
            s.background_texture = s.add_texture_checkerboard(a, s.add_texture_image_map(third), 4.0, 6.0)
        elif background == "scale":
            s.background_texture = s.add_texture_scale(a, s.add_texture_image_map(third))
    return s


_rays = {}


def env_rays(geometry):
    """gbuffer_reference.reference_samples of the frames ENV_FRAMES, one entry each (the background does not move a ray), once per process."""
    if geometry not in _rays:
        import gbuffer_reference as gr
        import kernel_matrix as km
        from oracle import oracle as oracle_mod
        o = oracle_mod.Oracle(env_scene(geometry, "solid"))
        _rays[geometry] = {f: gr.reference_samples(oracle_mod, o, km.W, km.H, f, 1, edges=False)["samples"][0] for f in ENV_FRAMES}
    return _rays[geometry]
