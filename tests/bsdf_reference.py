"""Test helper (not a conftest): the BSDF code -- compute_bsdf, the lobes' f / pdf / sample_f, the Trowbridge-Reitz functions, the two Fresnel
terms, Bsdf::f / pdf / sample_f -- in numpy and float64, vectorised over samples.  Written from the specification: the reference project's
material.rs, reflection.rs, reflection/{bxdf,microfacet,fresnel,onb}.rs, math.rs and rand.rs (each function below cites the lines it follows),
the comments that cite them in rene_amd/csrc/device_code.inc and the quirk list of SURVEY.md section 8 a -- not from the kernel's arithmetic
and not from oracle/rene_oracle.cpp.  Quirks kept: Q8 (Plastic never remaps its roughness, and its Fresnel is dielectric(1.5, 1)), Q9
(Beckmann's Lambda next to the Trowbridge-Reitz D), Q11 (sample11's g1 = 2 / (1 + (1 + 1 / sqrt(a0 a0)))), Bsdf::sample_f returning the chosen
lobe's own f and pdf / len.  Q1 (the integrator calls pdf(wi, normal)) lives in the caller: pdf here takes any two directions.  Rust's
f32::max / min ignore a NaN operand, so np.fmax / np.fmin stand where the specification has them.  Literals are the specification's fp32
literals (0.9999, 1.6, 1e-3, the polynomial coefficients, pi): a threshold is compared as the fp32 number it is.

Inputs are exact: the fp32 normal, uv, wo, wi, material parameters, texels (through texture_reference.tex_color), and the random numbers,
integers out of a numpy restatement of PCG32si (rand.rs:4-52, checked against tests/golden/pcg32si_kat.json); next_f32 = (u32 >> 8) 2^-24
is exact in float64.

  evaluate(scene, material, n, uv, wo, wi)   -> Eval: f (n, 3), pdf, len, their allowances, `aside` per quantity, the decisions
  sample(scene, material, n, uv, wo, seeds)  -> Sample: wi (world), f, pdf, len, draws, allowances, `aside`, and `dec`: every discrete decision
                                                the sample took as name -> (taken, value, margin).  Names: lobe (the index; margin: none, it is an
                                                integer), coin<F, coin<0.5, cos>0.9999, a<0||s2>a0, u2>0.5, tmp capped, dot(wo,wh)<0, same_hemisphere, flip, sin_theta==0,
                                                wo.z<0, wo.z>0, wo.z==0, sin2_t>=1, sin_t>=1, cos>0, a>=1.6, isinf(tan2), isinf(tan), zero, reflect

THE ALLOWANCE -- how far an fp32 evaluation of the same specification may lie from this one.  It comes from this reference's own sensitivity
and from operation counts, never from a device's or the oracle's output.  u = 2^-24 (half an fp32 ulp: one correctly rounded operation).
device_math.h states v_rcp_f32, v_rsq_f32, v_sqrt_f32 at 1 ulp (2 u) and qdiv at 2 ulp (4 u).

(a) The vectors an fp32 evaluation rounds are moved by +- BUDGET u per component, with N_PATTERNS fixed, seeded sign patterns, and the largest
    change of the fp64 result is taken.  BUDGET, first order, worst case, for unit vectors:
      n^ = n rsq(n.n): n.n 3 u relative (positive terms), halved by the root 1.5 u, rsq 2 u, the product 1 u: 4.5 u per component, relative;
      onb (math.rs:89-97): r = 1 / sqrt(y^2 + z^2): squares 10 u, sum 11 u, root 5.5 + 2 u, rcp 2 u = 9.5 u; a component of u: 4.5 + 9.5 + 1 =
      15 u relative; of v = w x u (each a difference of products that here has one sign): 4.5 + 15 + 1 + 1 = 21.5 u relative;
      to_local: a dot product's own roundings are 3 u sum|a_k b_k| <= 3 u, so z = a.w: 7.5 u, x = a.u: 18 u, y = a.v: 24.5 u.
    BUDGET_Z = 8 (7.5 rounded up) and BUDGET_XY = 26 (the y component's 24.5 rounded up to the next even number; x takes y's) for the local wo, wi;
    BUDGET_HALF = 6 (5.5 rounded up) for a vector normalised in the local frame -- the half vector normalize(wo + wi) (sum 1 u, normalize 4.5 u), sample_wh's
    stretched wo (a product 1 u, normalize 4.5 u) and its wh (4.5 u) -- and BUDGET_REFLECT = 9 for the reflected -wo + 2 (wo.wh) wh (the dot
    product 3 u, doubled; the product 2 u; the sum 1 u) and the refracted wi (less: its dot product with (0, 0, +-1) is exact), each on top of what
    their perturbed arguments bring.
(b) N u |result| for the scalar operations behind them, N counted per lobe kind from the formula (the N_* table below, each with its count).
(c) Parameters that are computed: roughness_to_alpha's alpha moves by its polynomial's roundings (logf taken at the OpenCL bound of 3 ulp =
    6 u on x, k products per term: u sum_k (7 k + 5) |c_k x^k|, large against alpha where the terms cancel), a textured parameter by
    texture_reference.tex_allowance, alpha behind a textured roughness by both.
(d) v_sin_f32 / v_cos_f32 carry an absolute error.  Neither the CDNA guides on hand nor the ROCm headers state a bound for them (both were
    searched), so TRIG_ABS = 2^-11 is ASSUMED: it is the bound the Vulkan specification sets for sin and cos on [-pi, pi], that is what
    the reference project's own shaders are entitled to on their platform.  cos(2 pi u), sin(2 pi u) each move by +- TRIG_ABS before they
    are scaled (random_cosine_direction, math.rs:45-56; sample11's cos_theta > 0.9999 branch, microfacet.rs:81-86).
(e) The sampled wi goes back to world space through the basis vectors (15, 21.5, 4.5 u) and three products and two sums: at most 21.5 u sum|wi_k b_k| + 3 u = 24.5 u, rounded up as BUDGET_XY: + 26 u per component.
(f) What fp32 computes exactly is not moved.  Where the normal is an axis, n^ and the frame are exact (n.n = 1, rsq(1) = 1, the frame's entries
    are 0 and +-1) and to_local selects and negates components: the local wo and wi are the inputs' own numbers.  Normalising an axis vector is
    exact likewise: a half vector or a stretched wo that is an axis is not moved, and its sin_theta == 0 (onb.rs:56-72) is safe.  The edge rows
    rest on this: with n = +z their `wo.z == 0`, `wo == n` and `wi the mirror of wo` are exact on the device too.

For scale: a wrong branch (the other root of sample11, a lobe's pdf on the wrong side), a missing abs, a missing face_forward or swapped
indices of refraction move f or pdf by 10 % to a factor of several (Fresnel at 1.5: 0.04 against 1.0 under total internal reflection); the
allowance of a well-conditioned sample is 1e-5 to 1e-4 of the result (N u is 1.3e-5 for the longest formula) and 5e-4 on a direction that
went through a sine and cosine.

SET-ASIDE.  A sample says little where its allowance exceeds 0.1 |reference| + 1e-6 (per quantity; any channel for a colour), or where one
of its perturbed evaluations takes a discrete decision the unperturbed one did not, or where the number a decision compares lies within its
own roundings of the threshold (the `slack` next to each note): it is set aside for that quantity (a decision sets aside all quantities of that
call). fr_dielectric's two decisions are recorded but set nothing aside: F is 1 on both sides of cos = 0 and of sin_t = 1.  The caps: SET_ASIDE_CAP =
5 % per case and quantity on the uniform and grazing sets, 0 on the edge set apart from EDGE_EXEMPT below. The caps are conditions on the inputs,
asserted from the reference alone in tests/test_bsdf_reference.py.  An
exemption in EDGE_EXEMPT names rows, quantities and -- where its reason holds for some cases only -- cases, and takes them out of the cap's count
alone: check() compares every sample to the allowance unless the reference's own rule set that very sample aside, and then still by class.
Where a case could not meet its cap its inputs changed, not the cap: GRAZING_WO_MIN raises the lower end of |cos(wo)| on the grazing set for the
cases with a specular lobe (to 2^-18.5, 2^-15) and with Uber's opacity lobe (to 2^-11.5, 2^-10.5), for the reasons written there; |cos(wi)|
keeps [2^-20, 2^-3] everywhere.  The alpha = 0.01 plate meets its cap on the uniform set as it stands (3.8 % of its sampled f and pdf).

The second half holds what the CPU and the GPU tests share: the scene (one quad instance per material, so the probe finds an instance and
takes the record a render would use) and the input sets -- uniform (2 048: random normals, wo and wi uniform on the sphere, nothing left
out by angle), grazing (1 024: |cos| log-uniform in [2^-20, 2^-3] for wo, wi or both) and the named edge rows."""
import functools

import numpy as np

import texture_reference as tr
from rene_amd import abi, glam
from rene_amd.scene import Scene, TriangleMesh

EPS = 2.0 ** -24
BUDGET_XY, BUDGET_Z, BUDGET_HALF, BUDGET_REFLECT = 26.0, 8.0, 6.0, 9.0  # 24.5, 7.5 and 5.5 rounded up to even numbers; 9 as counted
BUDGET_WORLD = 26.0
TRIG_ABS = 2.0 ** -11
N_PATTERNS = 16
SET_ASIDE_REL, SET_ASIDE_ABS, SET_ASIDE_CAP = 0.1, 1e-6, 0.05

# N of (b), in u.  Counted along the longest chain of each formula; a factor that enters squared counts twice.
#   D (microfacet.rs:141-155): tan2 = sin2 / cos2: 2 + 1 + 4; cos2_phi, sin2_phi: (root 2 + quotient 4) twice = 12; / alpha^2: 1 + 4; the sum and
#   the product by tan2: 2 => e: 26, (1 + e)^2: 54; cos4: 3; four products 4; the reciprocal 2                                     => 63
#   Lambda (157-174): tan 6, alpha (12 + 4 + 1) / 2 + 2 = 11, a: 1 + 2, the rational 2 (5) + 4 = 14, entering twice (a, a^2)          => 48
N_D, N_LAMBDA = 63, 48
N_FR_DIELECTRIC = 40  # bxdf.rs:138-165: sin_i 4, eta_i / eta_t 4, sin_t 1, cos_t 4, then (difference over sum of products) 2 + 1 + 4, squared twice, sum, half
N_FR_CONDUCTOR = 64   # fresnel.rs:78-102: two quotients 6, eta2 .. t0 5, a2plusb2 6 + 2, a 3 + 2, t1 t2 4, rs 6, t3 t4 6, rp 8, sum 2; differences of like terms doubled
N = {
    "lambert.f": 2,        # bxdf.rs:87-89: one product
    "lambert.pdf": 6,      # 107-113: one product; / len 4
    "blend.f": 112,        # 266-290: diffuse 2 + 2 + 2 (8 + 1) + 2 = 24; specular D 63 + dot 3 + 4 |c| max 3 + quotient 4 + schlick 12 + product 1 = 86; the sum 2
    "blend.pdf": 136,      # 319-328: D 63 + g1 (Lambda 48 + 1 + 2) + |dot| 3 + product 2 + quotient 4 = 123; / (4 dot) 5; sum with cos / pi, half: 4; / len 4
    "micro.f": 240,        # 361-383: D 63 + G (2 Lambda 96 + 2 + 2) + Fresnel 64 + dot 3 + 4 ci co 2 + three products 3 + quotient 3 = 238
    "micro.pdf": 136,      # 407-414: as blend.pdf without the sum
    "fresnel_specular": 50,  # 193-227: Fresnel 40 + 1 - F 1 + quotient 4 (+ eta_i / eta_t 4)
    "mirror": 6,           # 437-443: product, quotient 4
    "spec_refl": 48,       # the same with a dielectric Fresnel
    "spec_trans": 56,      # 481-512: Fresnel 40 on the refracted cosine + 1 - F + product + quotient 4, eta_i / eta_t 4
}

FR_CONDUCTOR, FR_NOOP, FR_DIELECTRIC = range(3)  # fresnel.rs:16-20
LAMBERT, FRESNEL_SPECULAR, FRESNEL_BLEND, MICROFACET, SPEC_REFL, SPEC_TRANS = range(6)  # reflection.rs:106-113
_DIFFUSE_REFLECTION = (LAMBERT, FRESNEL_BLEND, MICROFACET)  # kind() holds REFLECTION: bxdf.rs:83, 262, 357 (FresnelSpecular's f is zero)


def c32(v):
    """An fp32 literal of the specification as the number it is."""
    return float(np.float32(v))


PI, INV_PI, C9999, C16 = c32(np.pi), c32(1.0 / np.pi), c32(0.9999), c32(1.6)
_IGNORE = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


# ---- PCG32si, rand.rs:4-52, in integers ------------------------------------------------------------------------------------------------------------------
M32 = 0xFFFFFFFF
_MUL, _INC, _OUT = 747796405, 2891336453, 277803737


def _step(s):
    return (s * np.uint64(_MUL) + np.uint64(_INC)) & np.uint64(M32)


def _output(s):  # rand.rs:19-22
    word = (((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(_OUT)) & np.uint64(M32)
    return (word >> np.uint64(22)) ^ word


def pcg_new(seed):  # rand.rs:24-30
    seed = np.atleast_1d(np.asarray(seed)).astype(np.uint64) & np.uint64(M32)
    return _step((_step(seed) + seed) & np.uint64(M32))


class Rng:
    """One generator per sample; a draw advances only the samples in `idx`.  draws: how many numbers each sample has consumed."""

    def __init__(self, seeds, skip=0):
        self.state = pcg_new(seeds)
        for _ in range(skip):  # numbers the caller's stream has consumed before (a pixel's two jitter draws)
            self.state = _step(self.state)
        self.draws = np.zeros(len(self.state), np.int64)

    def u32(self, idx):  # rand.rs:32-36
        s = self.state[idx]
        self.state[idx] = _step(s)
        self.draws[idx] += 1
        return _output(s)

    def f32(self, idx):  # rand.rs:38-47
        return (self.u32(idx) >> np.uint64(8)).astype(np.float64) * EPS


def _unoutput(o):
    w = o ^ (o >> 22)
    w = (w * pow(_OUT, -1, 1 << 32)) & M32
    rs, x = 4 + (w >> 28), w  # the top four bits pass through the xorshift, so the shift is known
    for _ in range(8):
        x = w ^ (x >> rs)
    return x


def _unstep(s):
    return ((s - _INC) * pow(_MUL, -1, 1 << 32)) & M32


def seed_with(first=None, second=None):
    """A seed whose first (or second) next_u32 lies in the given range: the output permutation and the LCG are inverted; new() maps a seed to
    step(seed (MUL + 1) + INC), and MUL + 1 is even, so only every other state has a seed (two of them)."""
    rng, second_draw = (first, False) if first is not None else (second, True)
    for t in rng:
        s0 = _unoutput(t)
        if second_draw:
            s0 = _unstep(s0)
        r = (_unstep(s0) - _INC) & M32
        if r % 2 == 0:
            seed = (r // 2 * pow((_MUL + 1) // 2, -1, 1 << 31)) % (1 << 31)
            got = _output(pcg_new(seed) if not second_draw else _step(pcg_new(seed)))
            assert int(got[0]) == t
            return seed
    raise ValueError("no seed")


# ---- decisions ---------------------------------------------------------------------------------------------------------------------------------------------
class Decisions:
    """name -> [taken, value, margin], each (n,): which samples reached the decision, what it decided, how far the deciding number was from the
    threshold (NaN where the decision is an integer's)."""

    def __init__(self, n):
        self.n, self.items, self.unsafe, self.continuous = n, {}, np.zeros(n, bool), set()

    def note(self, name, idx, value, margin=None, slack=None, continuous=False):
        """slack: the roundings of the number that is compared, in its own units; a margin inside it marks the sample unsafe."""
        if continuous:
            self.continuous.add(name)
        e = self.items.get(name)
        if e is None:
            e = self.items[name] = [np.zeros(self.n, bool), np.zeros(self.n, np.int64), np.full(self.n, np.nan)]
        e[0][idx] = True
        e[1][idx] = value
        if margin is not None:
            e[2][idx] = margin
            if slack is not None:
                self.unsafe[idx] |= ~(margin >= slack)

    def differs(self, other):
        out = np.zeros(self.n, bool)
        for name in (set(self.items) | set(other.items)) - self.continuous - other.continuous:
            a, b = self.items.get(name), other.items.get(name)
            if a is None or b is None:
                out |= (a or b)[0]
            else:
                out |= (a[0] != b[0]) | (a[0] & (a[1] != b[1]))
        return out


# ---- onb.rs ------------------------------------------------------------------------------------------------------------------------------------------------
def onb_from_w(w):
    """Onb::from_w, onb.rs:14-18, over coordinate_system, math.rs:89-97: the first form where |x| > |y| (a tie takes the second)."""
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    first = np.abs(x) > np.abs(y)
    zero = np.zeros_like(x)
    with np.errstate(**_IGNORE):
        u = np.where(first[:, None], np.stack([-z, zero, x], -1) / np.sqrt(x * x + z * z)[:, None],
                     np.stack([zero, z, -y], -1) / np.sqrt(y * y + z * z)[:, None])
    return u, np.cross(w, u), w


def _sin2(w):  # onb.rs:40-42
    return np.fmax(1.0 - w[:, 2] * w[:, 2], 0.0)


def _phi(w, dec=None, idx=None, tag=""):
    """local_cos_phi, local_sin_phi, onb.rs:56-72: (1, 0) where sin_theta == 0.  Where it is noted as a decision (sample_wh's stretched wo, whose
    azimuth turns the sampled slope), sin2_theta = 1 - z^2 within 2 BUDGET_HALF u of 0 is within the roundings of z: unsafe."""
    s = np.sqrt(_sin2(w))
    if dec is not None:
        dec.note(tag + "sin_theta==0", idx, s == 0, _sin2(w), np.where(_axis(w), 0.0, 2 * BUDGET_HALF * EPS))
    with np.errstate(**_IGNORE):
        return np.where(s == 0, 1.0, np.clip(w[:, 0] / s, -1.0, 1.0)), np.where(s == 0, 0.0, np.clip(w[:, 1] / s, -1.0, 1.0))


def _axis(v):
    """Vectors whose components are all 0 or +-1 ((f) of the module docstring)."""
    return ((v == 0) | (np.abs(v) == 1)).all(-1)


def _moved_unit(v, d):
    """normalize(v), moved by d unless it is an axis."""
    v = _unit(v)
    return v + np.where(_axis(v)[:, None], 0.0, d)


def _unit(v):
    with np.errstate(**_IGNORE):
        return v / np.sqrt((v * v).sum(-1))[:, None]


def _dot(a, b):
    return (a * b).sum(-1)


# ---- fresnel.rs, bxdf.rs:138-165 -----------------------------------------------------------------------------------------------------------------------
def fr_dielectric(cos_i, eta_i, eta_t, dec=None, idx=None, tag="", scal=None):
    """bxdf.rs:138-165: the indices swap where cos <= 0; 1 past the critical angle."""
    scal = scal or _NO_SCALAR_MOVES
    cos_i = np.clip(np.asarray(cos_i, np.float64), -1.0, 1.0)
    eta_i, eta_t = np.broadcast_to(np.float64(eta_i), cos_i.shape), np.broadcast_to(np.float64(eta_t), cos_i.shape)
    entering = cos_i > 0
    ei, et = np.where(entering, eta_i, eta_t), np.where(entering, eta_t, eta_i)
    c = np.abs(cos_i)
    with np.errstate(**_IGNORE):
        sin_t = ei / et * np.sqrt(np.fmax(1.0 - c * c + scal["1-c2"], 0.0))
        tir = sin_t >= 1.0
        cos_t = np.sqrt(np.fmax(1.0 - sin_t * sin_t + scal["1-st2"] * np.fmax(1.0, sin_t * sin_t), 0.0))
        r_parl = (et * c - ei * cos_t) / (et * c + ei * cos_t)
        r_perp = (ei * c - et * cos_t) / (ei * c + et * cos_t)
    if dec is not None:  # recorded, but F is continuous across both (1 at cos = 0 and at sin_t = 1): a flip sets nothing aside
        dec.note(tag + "cos>0", idx, entering, c, continuous=True)
        dec.note(tag + "sin_t>=1", idx, tir, np.abs(sin_t - 1.0), continuous=True)
    return np.where(tir, 1.0, 0.5 * (r_parl * r_parl + r_perp * r_perp))


def fr_conductor(cos_i, eta_t, k):
    """fresnel.rs:78-102 with eta_i = 1 (material.rs:298-302); cos_i (n,), eta_t and k (n, 3)."""
    c = np.clip(cos_i, -1.0, 1.0)[:, None]
    c2 = c * c
    s2 = 1.0 - c2
    eta2, k2 = eta_t * eta_t, k * k
    t0 = eta2 - k2 - s2
    with np.errstate(**_IGNORE):
        a2plusb2 = np.sqrt(t0 * t0 + 4.0 * eta2 * k2)
        t1 = a2plusb2 + c2
        a = np.sqrt(0.5 * (a2plusb2 + t0))
        t2 = 2.0 * c * a
        rs = (t1 - t2) / (t1 + t2)
        t3 = c2 * a2plusb2 + s2 * s2
        t4 = t2 * s2
        rp = rs * (t3 - t4) / (t3 + t4)
    return 0.5 * (rp + rs)


def _fresnel(l, cos_i, dec, idx, tag, scal=None):
    """EnumFresnel::evaluate, fresnel.rs:160-171; the conductor takes |cos| (104-108)."""
    if l["fr"] == FR_NOOP:
        return np.ones((len(cos_i), 3))
    if l["fr"] == FR_CONDUCTOR:
        return fr_conductor(np.abs(cos_i), l["eta3"], l["k3"])
    return np.repeat(fr_dielectric(cos_i, l["eta_i"], l["eta_t"], dec, idx, tag, scal)[:, None], 3, 1)


# ---- microfacet.rs ---------------------------------------------------------------------------------------------------------------------------------------
_RC = [c32(v) for v in (1.62142, 0.819955, 0.1734, 0.0171201, 0.000640711)]


def roughness_to_alpha(r):
    """microfacet.rs:65-74."""
    x = np.log(np.fmax(np.asarray(r, np.float64), c32(1e-3)))
    return sum(c * x ** k for k, c in enumerate(_RC))


def alpha_error(r, dr):
    """(c) of the module docstring: the polynomial's own roundings and the slope times the roughness's error (0 under the clamp)."""
    r = np.asarray(r, np.float64)
    x = np.log(np.fmax(r, c32(1e-3)))
    own = EPS * sum((7 * k + 5) * np.abs(c * x ** k) for k, c in enumerate(_RC))
    slope = np.abs(sum(k * c * x ** (k - 1) for k, c in enumerate(_RC) if k)) / np.fmax(r, c32(1e-3))
    return own + np.where(r > c32(1e-3), slope, 0.0) * dr


def tr_d(ax, ay, wh, dec=None, idx=None, tag=""):
    """microfacet.rs:141-155."""
    with np.errstate(**_IGNORE):
        c2 = wh[:, 2] * wh[:, 2]
        t2 = _sin2(wh) / c2
        inf = np.isinf(t2)
        cp, sp = _phi(wh)
        e = (cp * cp / (ax * ax) + sp * sp / (ay * ay)) * t2
        d = 1.0 / (PI * ax * ay * (c2 * c2) * (1.0 + e) * (1.0 + e))
    if dec is not None:
        dec.note(tag + "isinf(tan2)", idx, inf, np.abs(wh[:, 2]))
    return np.where(inf, 0.0, d)


def tr_lambda(ax, ay, w, dec=None, idx=None, tag=""):
    """microfacet.rs:157-174 (Q9: Beckmann's fit)."""
    with np.errstate(**_IGNORE):
        abs_tan = np.abs(np.sqrt(_sin2(w)) / w[:, 2])
        inf = np.isinf(abs_tan)
        cp, sp = _phi(w)
        a = 1.0 / (np.sqrt(cp * cp * ax * ax + sp * sp * ay * ay) * abs_tan)
        big = a >= C16
        lam = (1.0 - c32(1.259) * a + c32(0.396) * a * a) / (c32(3.535) * a + c32(2.181) * a * a)
    if dec is not None:
        dec.note(tag + "isinf(tan)", idx, inf, np.abs(w[:, 2]))
        dec.note(tag + "a>=1.6", idx[~inf], big[~inf], np.abs(a - C16)[~inf], 20 * EPS * C16)  # tan 6 u, alpha 11 u, the product and the reciprocal 3 u
    return np.where(inf | big, 0.0, lam)


def tr_pdf(ax, ay, wo, wh, dec, idx, tag):
    """microfacet.rs:192-194 with g1 of 20-22."""
    with np.errstate(**_IGNORE):
        return tr_d(ax, ay, wh, dec, idx, tag + "D.") * (1.0 / (1.0 + tr_lambda(ax, ay, wo, dec, idx, tag + "L(wo)."))) * np.abs(_dot(wo, wh)) / np.abs(wo[:, 2])


def sample11(cos_t, u1, u2, trig, m, dec, idx, tag):
    """trowbridge_reitz_sample11, microfacet.rs:77-122 (Q11 in g1)."""
    near = cos_t > C9999
    with np.errstate(**_IGNORE):
        r = np.sqrt(u1 / (1.0 - u1))
        ax_, ay_ = r * (np.cos(2.0 * np.pi * u2) + trig[:, 0]), r * (np.sin(2.0 * np.pi * u2) + trig[:, 1])
        sin_t = np.sqrt(np.fmax(1.0 - cos_t * cos_t, 0.0))
        tan_t = sin_t / cos_t
        a0 = 1.0 / tan_t
        g1 = 2.0 / (1.0 + (1.0 + 1.0 / np.sqrt(a0 * a0)))
        a = 2.0 * u1 / g1 - 1.0
        raw = 1.0 / (a * a - 1.0)
        capped, pole = ~(raw < c32(1e10)), np.abs(a * a - 1.0)  # min(1 / (a^2 - 1), 1e10): the cap holds where a^2 - 1 is 0 (u1 = 0) or below 1e-10
        a = a + m[:, 0] * (1.0 + np.abs(a))
        tmp = np.fmin(1.0 / (a * a - 1.0), c32(1e10))
        b = tan_t
        t1, t2 = b * b * tmp * tmp, (a * a - b * b) * tmp
        d = np.sqrt(np.fmax(t1 - t2 + m[:, 1] * (np.abs(t1) + np.abs(t2)), 0.0))
        s1, s2 = b * tmp - d, b * tmp + d
        first = (a < 0) | (s2 > a0)
        sx = np.where(first, s1, s2) + m[:, 2] * (np.abs(b * tmp) + d)
        up = u2 > 0.5
        v = np.where(up, 2.0 * (u2 - 0.5), 2.0 * (0.5 - u2))
        z = ((v * (v * (v * c32(0.27385) - c32(0.73369)) + c32(0.46341))) + m[:, 5]) / (v * (v * (v * c32(0.093073) + c32(0.309420)) - 1.0) + c32(0.597999) + m[:, 6])
        sy = np.where(up, 1.0, -1.0) * z * np.sqrt(1.0 + sx * sx)
    dec.note(tag + "cos>0.9999", idx, near, np.abs(cos_t - C9999), 6 * EPS)
    far = ~near
    dec.note(tag + "a<0||s2>a0", idx[far], first[far], np.fmin(np.abs(a), np.abs(s2 - a0))[far], 64 * EPS * (1.0 + np.abs(a0))[far])  # g1 12 u, a 6 u; tmp, d, s2: 40 u = 58 u, rounded up to the next power of two
    dec.note(tag + "u2>0.5", idx[far], up[far], np.abs(u2 - 0.5)[far])
    # a^2 - 1 carries 2 |a| times a's 16 u (1 + |a|); inside that, tmp is the cap or a huge number of either sign and slope_x = b tmp - d cancels all of it
    dec.note(tag + "tmp capped", idx[far], capped[far], pole[far], (32 * EPS * np.abs(a) * (1.0 + np.abs(a)) + 2 * EPS)[far])
    return np.where(near, ax_, sx) * (1.0 + m[:, 3]), np.where(near, ay_, sy) * (1.0 + m[:, 4])


def sample_wh(l, wo, rng, idx, P, dec, tag):
    """TrowbridgeReitz::sample_wh, microfacet.rs:176-190, over trowbridge_reitz_sample, 124-138."""
    ax, ay = l["ax"], l["ay"]
    flip = wo[:, 2] < 0
    dec.note(tag + "flip", idx, flip, np.abs(wo[:, 2]))
    w = np.where(flip[:, None], -wo, wo)
    ws = _moved_unit(np.stack([ax * w[:, 0], ay * w[:, 1], w[:, 2]], -1), P["s_ws"])
    u1, u2 = rng.f32(idx), rng.f32(idx)
    sx, sy = sample11(ws[:, 2], u1, u2, P["trig"], P["s11"], dec, idx, tag)
    cp, sp = _phi(ws, dec, idx, tag)
    with np.errstate(**_IGNORE):
        wh = _unit(np.stack([-ax * (cp * sx - sp * sy), -ay * (sp * sx + cp * sy), np.ones_like(sx)], -1)) + P["s_wh"]
    return np.where(flip[:, None], -wh, wh)


# ---- bxdf.rs -----------------------------------------------------------------------------------------------------------------------------------------------
def _pow5(v):
    return (v * v) * (v * v) * v


def _same_hemisphere(a, b, dec, idx, tag):  # onb.rs:84-86
    same = a[:, 2] * b[:, 2] > 0
    dec.note(tag + "same_hemisphere", idx, same, np.fmin(np.abs(a[:, 2]), np.abs(b[:, 2])))
    return same


class Moves:
    """What a lobe's f and pdf are moved by: the half vector's move (n, 3) and the scalar moves of the pattern in force."""

    def __init__(self, wh, scal=None):
        self.wh, self.scal = wh, scal

    def __getitem__(self, k):
        return Moves(self.wh[k], self.scal)


def _half(wo, wi, dwh):
    wh = wi + wo
    return (wh == 0).all(-1), _moved_unit(wh, dwh.wh)


def lambert_pdf(l, wo, wi, dwh, dec, idx, tag):  # bxdf.rs:107-113
    return np.where(_same_hemisphere(wo, wi, dec, idx, tag), np.abs(wi[:, 2]) * INV_PI, 0.0)


def lambert_f(l, wo, wi, dwh, dec, idx, tag):  # bxdf.rs:87-89
    return l["a"] * INV_PI


def blend_f(l, wo, wi, dwh, dec, idx, tag):
    """FresnelBlend::f, bxdf.rs:266-290, schlick_fresnel 253-258."""
    ci, co = np.abs(wi[:, 2]), np.abs(wo[:, 2])
    diffuse = c32(28.0 / (23.0 * np.pi)) * l["a"] * (1.0 - l["b"]) * ((1.0 - _pow5(1.0 - 0.5 * ci)) * (1.0 - _pow5(1.0 - 0.5 * co)))[:, None]
    zero, wh = _half(wo, wi, dwh)
    dec.note(tag + "zero", idx, zero)
    c = _dot(wi, wh)
    schlick = l["b"] + _pow5(1.0 - c)[:, None] * (1.0 - l["b"])
    with np.errstate(**_IGNORE):
        specular = (tr_d(l["ax"], l["ay"], wh, dec, idx, tag + "D.") / (4.0 * np.abs(c) * np.fmax(ci, co)))[:, None] * schlick
    return np.where(zero[:, None], 0.0, diffuse + specular)


def blend_pdf(l, wo, wi, dwh, dec, idx, tag):  # bxdf.rs:319-328
    same = _same_hemisphere(wo, wi, dec, idx, tag)
    _, wh = _half(wo, wi, dwh)
    with np.errstate(**_IGNORE):
        p = 0.5 * (np.abs(wi[:, 2]) * INV_PI + tr_pdf(l["ax"], l["ay"], wo, wh, dec, idx, tag + "pdf.") / (4.0 * _dot(wo, wh)))
    return np.where(same, p, 0.0)


def micro_f(l, wo, wi, dwh, dec, idx, tag):
    """MicrofacetReflection::f, bxdf.rs:361-383; face_forward 348-354."""
    ci, co = np.abs(wi[:, 2]), np.abs(wo[:, 2])
    zero, wh = _half(wo, wi, dwh)
    zero = zero | (ci == 0) | (co == 0)
    dec.note(tag + "zero", idx, zero, np.fmin(ci, co))
    back = wh[:, 2] < 0
    if l["fr"] == FR_DIELECTRIC:
        dec.note(tag + "face_forward", idx, back, np.abs(wh[:, 2]))
    fr = _fresnel(l, _dot(wi, np.where(back[:, None], -wh, wh)), dec, idx, tag + "F.", dwh.scal)
    with np.errstate(**_IGNORE):
        g = 1.0 / (1.0 + tr_lambda(l["ax"], l["ay"], wo, dec, idx, tag + "L(wo).") + tr_lambda(l["ax"], l["ay"], wi, dec, idx, tag + "L(wi)."))  # microfacet.rs:16-18
        f = l["a"] * (tr_d(l["ax"], l["ay"], wh, dec, idx, tag + "D.") * g)[:, None] * fr / (4.0 * ci * co)[:, None]
    return np.where(zero[:, None], 0.0, f)


def micro_pdf(l, wo, wi, dwh, dec, idx, tag):  # bxdf.rs:408-414
    same = _same_hemisphere(wo, wi, dec, idx, tag)
    _, wh = _half(wo, wi, dwh)
    with np.errstate(**_IGNORE):
        p = tr_pdf(l["ax"], l["ay"], wo, wh, dec, idx, tag + "pdf.") / (4.0 * _dot(wo, wh))
    return np.where(same, p, 0.0)


def _zero_f(l, wo, wi, dwh, dec, idx, tag):  # bxdf.rs:189-191, 433-435, 477-479
    return np.zeros((len(wo), 3))


def _zero_pdf(l, wo, wi, dwh, dec, idx, tag):  # bxdf.rs:228-230, 445-447, 514-516
    return np.zeros(len(wo))


LOBE_F = {LAMBERT: lambert_f, FRESNEL_BLEND: blend_f, MICROFACET: micro_f, FRESNEL_SPECULAR: _zero_f, SPEC_REFL: _zero_f, SPEC_TRANS: _zero_f}
LOBE_PDF = {LAMBERT: lambert_pdf, FRESNEL_BLEND: blend_pdf, MICROFACET: micro_pdf, FRESNEL_SPECULAR: _zero_pdf, SPEC_REFL: _zero_pdf, SPEC_TRANS: _zero_pdf}
N_F = {LAMBERT: N["lambert.f"], FRESNEL_BLEND: N["blend.f"], MICROFACET: N["micro.f"]}
N_PDF = {LAMBERT: N["lambert.pdf"], FRESNEL_BLEND: N["blend.pdf"], MICROFACET: N["micro.pdf"]}
N_SAMPLE = {FRESNEL_SPECULAR: N["fresnel_specular"], SPEC_REFL: N["spec_refl"], SPEC_TRANS: N["spec_trans"]}


def reflect(wo, n):  # bxdf.rs:117-119
    return -wo + 2.0 * _dot(wo, n)[:, None] * n


def refract(wi, nz, eta, dec, idx, tag, scal=None):
    """bxdf.rs:121-136 with n = (0, 0, nz); returns ok and the direction ((0, 0, 0) where it fails)."""
    cos_i = nz * wi[:, 2]
    sin2_t = eta * eta * np.fmax(1.0 - cos_i * cos_i, 0.0)
    fail = sin2_t >= 1.0
    moved = sin2_t + (scal or _NO_SCALAR_MOVES)["sin2_t"] * np.fmax(1.0, eta * eta)  # the decision keeps the unmoved number: its slack is the note's
    dec.note(tag + "sin2_t>=1", idx, fail, np.abs(sin2_t - 1.0), 12 * EPS)  # 1 - cos^2 2 u, eta 4 u entering squared, two products: of a number near 1
    with np.errstate(**_IGNORE):
        cos_t = np.sqrt(np.fmax(1.0 - moved, 0.0))
        out = eta[:, None] * -wi
        out[:, 2] += (eta * cos_i - cos_t) * nz
    return ~fail, np.where(fail[:, None], 0.0, out)


def _mirror(wo):
    return wo * np.float64([-1.0, -1.0, 1.0])


def _cosine_direction(wo, rng, idx, P, dec, tag):
    """random_cosine_direction, math.rs:45-56, turned to wo's side (bxdf.rs:92-96, 294-298)."""
    r1, r2 = rng.f32(idx), rng.f32(idx)
    s = np.sqrt(r2)
    wi = np.stack([(np.cos(2.0 * np.pi * r1) + P["trig"][:, 0]) * s, (np.sin(2.0 * np.pi * r1) + P["trig"][:, 1]) * s, np.sqrt(1.0 - r2)], -1)
    below = wo[:, 2] < 0
    dec.note(tag + "wo.z<0", idx, below, np.abs(wo[:, 2]))
    wi[:, 2] = np.where(below, -wi[:, 2], wi[:, 2])
    return wi + P["s_wi"]


def _sample_lambert(l, wo, rng, idx, P, dec, tag):  # bxdf.rs:91-105
    wi = _cosine_direction(wo, rng, idx, P, dec, tag)
    return wi, lambert_f(l, wo, wi, None, dec, idx, tag), lambert_pdf(l, wo, wi, None, dec, idx, tag)


def _sample_fresnel_specular(l, wo, rng, idx, P, dec, tag):  # bxdf.rs:193-227
    ir = l["a"][:, 0]
    fr = fr_dielectric(wo[:, 2], 1.0, ir, dec, idx, tag + "F.", P["scal"])
    u = rng.f32(idx)
    refl = u < fr
    dec.note(tag + "coin<F", idx, refl, np.abs(u - fr), N_FR_DIELECTRIC * EPS * fr)
    up = wo[:, 2] > 0
    dec.note(tag + "wo.z>0", idx[~refl], up[~refl], np.abs(wo[:, 2])[~refl])
    ok, wt = refract(wo, np.where(up, 1.0, -1.0), np.where(up, 1.0 / ir, ir / 1.0), dec, idx, tag, P["scal"])
    wt = wt + np.where(ok[:, None], P["s_wi"], 0.0)
    wi = np.where(refl[:, None], _mirror(wo), wt)
    with np.errstate(**_IGNORE):
        f = np.where(refl, fr, 1.0 - fr) / np.abs(wi[:, 2])
    return wi, np.repeat(f[:, None], 3, 1), np.where(refl, fr, np.where(ok, 1.0 - fr, 0.0))


def _default(n):
    return np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)


def _sample_blend(l, wo, rng, idx, P, dec, tag):  # bxdf.rs:292-317
    n = len(wo)
    u = rng.f32(idx)
    diffuse = u < 0.5
    dec.note(tag + "coin<0.5", idx, diffuse, np.abs(u - 0.5))
    wi, keep = np.zeros((n, 3)), np.ones(n, bool)
    a, b = np.nonzero(diffuse)[0], np.nonzero(~diffuse)[0]
    if len(a):
        wi[a] = _cosine_direction(wo[a], rng, idx[a], _sub(P, a), dec, tag)
    if len(b):
        wh = sample_wh(_sub(l, b), wo[b], rng, idx[b], _sub(P, b), dec, tag)
        wi[b] = reflect(wo[b], wh) + P["s_wi"][b]
        keep[b] = _same_hemisphere(wo[b], wi[b], dec, idx[b], tag + "wh.")
    k = np.nonzero(keep)[0]
    out = _default(n)
    out[0][k] = wi[k]
    out[1][k] = blend_f(_sub(l, k), wo[k], wi[k], Moves(P["s_whe"][k], P["scal"]), dec, idx[k], tag + "f.")
    out[2][k] = blend_pdf(_sub(l, k), wo[k], wi[k], Moves(P["s_whe"][k], P["scal"]), dec, idx[k], tag + "p.")
    return out


def _sample_micro(l, wo, rng, idx, P, dec, tag):  # bxdf.rs:385-406
    n = len(wo)
    out = _default(n)
    flat = wo[:, 2] == 0
    dec.note(tag + "wo.z==0", idx, flat, np.abs(wo[:, 2]))
    a = np.nonzero(~flat)[0]
    if not len(a):
        return out
    wh = sample_wh(_sub(l, a), wo[a], rng, idx[a], _sub(P, a), dec, tag)
    d = _dot(wo[a], wh)
    back = d < 0
    dec.note(tag + "dot(wo,wh)<0", idx[a], back, np.abs(d))
    a, wh = a[~back], wh[~back]
    wi = reflect(wo[a], wh) + P["s_wi"][a]
    same = _same_hemisphere(wo[a], wi, dec, idx[a], tag + "wh.")
    a, wh, wi = a[same], wh[same], wi[same]
    la = _sub(l, a)
    out[0][a] = wi
    with np.errstate(**_IGNORE):
        out[2][a] = tr_pdf(la["ax"], la["ay"], wo[a], wh, dec, idx[a], tag + "p.") / (4.0 * _dot(wo[a], wh))
    out[1][a] = micro_f(la, wo[a], wi, Moves(P["s_whe"][a], P["scal"]), dec, idx[a], tag + "f.")
    return out


def _sample_spec_refl(l, wo, rng, idx, P, dec, tag):  # bxdf.rs:437-443
    wi = _mirror(wo)
    with np.errstate(**_IGNORE):
        f = _fresnel(l, wi[:, 2], dec, idx, tag + "F.", P["scal"]) * l["a"] / np.abs(wi[:, 2])[:, None]
    return wi, f, np.ones(len(wo))


def _sample_spec_trans(l, wo, rng, idx, P, dec, tag):  # bxdf.rs:481-512
    n = len(wo)
    up = wo[:, 2] > 0
    dec.note(tag + "wo.z>0", idx, up, np.abs(wo[:, 2]))
    ea, eb = np.broadcast_to(np.float64(l["eta_i"]), (n,)), np.broadcast_to(np.float64(l["eta_t"]), (n,))
    ok, wi = refract(wo, np.where(up, 1.0, -1.0), np.where(up, ea / eb, eb / ea), dec, idx, tag, P["scal"])
    wi = wi + np.where(ok[:, None], P["s_wi"], 0.0)
    out = _default(n)
    k = np.nonzero(ok)[0]
    fr = fr_dielectric(wi[k, 2], ea[k], eb[k], dec, idx[k], tag + "F.", P["scal"])
    with np.errstate(**_IGNORE):
        out[1][k] = l["a"][k] * ((1.0 - fr) / np.abs(wi[k, 2]))[:, None]
    out[0][k], out[2][k] = wi[k], 1.0
    return out


LOBE_SAMPLE = {LAMBERT: _sample_lambert, FRESNEL_SPECULAR: _sample_fresnel_specular, FRESNEL_BLEND: _sample_blend, MICROFACET: _sample_micro,
               SPEC_REFL: _sample_spec_refl, SPEC_TRANS: _sample_spec_trans}


def _sub(d, k):
    return {name: (v[k] if isinstance(v, np.ndarray) else v) for name, v in d.items()}


# ---- material.rs: the lobes of a material at uv ----------------------------------------------------------------------------------------------------------
def _lobe(n, kind, **kw):
    l = dict(kind=kind, present=np.ones(n, bool), a=np.zeros((n, 3)), b=np.zeros((n, 3)), ax=np.zeros(n), ay=np.zeros(n), fr=FR_CONDUCTOR, eta_i=1.0,
             eta_t=1.0, eta3=np.zeros((n, 3)), k3=np.zeros((n, 3)), da=np.zeros(n), db=np.zeros(n), dax=np.zeros(n), day=np.zeros(n), deta=np.zeros(n),
             dk=np.zeros(n))
    l.update(kw)
    return l


def lobes(scene, material, uv):
    """EnumMaterial::compute_bsdf, material.rs:739-769: the lobes in the order they are added, each with `present` per sample (Uber and Plastic
    add a lobe only where its colour is not zero) and the errors of its parameters ((c) of the module docstring)."""
    m = scene.materials[material]
    uv = np.asarray(uv, np.float32).astype(np.float64)
    n = len(uv)

    def col(tex):
        return tr.tex_color(scene, int(tex), uv[:, 0], uv[:, 1]), np.broadcast_to(tr.tex_allowance(scene, int(tex), uv[:, 0], uv[:, 1]), (n,)).astype(np.float64)

    def alphas(tu, tv, remap):
        (ru, du), (rv, dv) = col(tu), col(tv)
        ru, rv = ru[:, 0], rv[:, 0]
        if remap:
            return roughness_to_alpha(ru), roughness_to_alpha(rv), alpha_error(ru, du), alpha_error(rv, dv)
        return ru, rv, du, dv

    t = m.type
    if t == abi.MATERIAL_MATTE:  # material.rs:127-135
        a, da = col(m.u0[0])
        return [_lobe(n, LAMBERT, a=a, da=da)]
    if t == abi.MATERIAL_GLASS:  # 342-350
        return [_lobe(n, FRESNEL_SPECULAR, a=np.full((n, 3), float(m.v0[0])) * np.float64([1, 0, 0]))]
    if t == abi.MATERIAL_SUBSTRATE:  # 188-216
        (a, da), (b, db) = col(m.u0[0]), col(m.u0[1])
        ax, ay, dax, day = alphas(m.u0[2], m.u0[3], m.u1[0] != 0)
        return [_lobe(n, FRESNEL_BLEND, a=a, da=da, b=b, db=db, ax=ax, ay=ay, dax=dax, day=day)]
    if t == abi.MATERIAL_METAL:  # 279-307
        (eta, deta), (k, dk) = col(m.u0[0]), col(m.u0[1])
        ax, ay, dax, day = alphas(m.u0[2], m.u0[3], m.u1[0] != 0)
        return [_lobe(n, MICROFACET, a=np.ones((n, 3)), ax=ax, ay=ay, dax=dax, day=day, fr=FR_CONDUCTOR, eta3=eta, k3=k, deta=deta, dk=dk)]
    if t == abi.MATERIAL_MIRROR:  # 363-373
        a, da = col(m.u0[0])
        return [_lobe(n, SPEC_REFL, a=a, da=da, fr=FR_NOOP)]
    if t == abi.MATERIAL_UBER:  # 579-630
        e = float(m.v0[0])
        op, dop = col(m.u1[0])
        out = []

        def add(kind, colour, dcol, **kw):
            out.append(_lobe(n, kind, a=colour, da=dcol, present=(colour != 0).any(-1), **kw))
        add(SPEC_TRANS, 1.0 - op, dop, eta_i=1.0, eta_t=1.0)
        add(LAMBERT, *col(m.u0[0]))
        ax, ay, dax, day = alphas(m.u1[2], m.u1[3], m.u1[1] != 0)
        add(MICROFACET, *col(m.u0[1]), ax=ax, ay=ay, dax=dax, day=day, fr=FR_DIELECTRIC, eta_i=1.0, eta_t=e)
        for tex, kind in ((m.u0[2], SPEC_REFL), (m.u0[3], SPEC_TRANS)):
            c, dc = col(tex)
            add(kind, op * c, dc * np.abs(op).max(-1) + dop * np.abs(c).max(-1) + EPS * np.abs(op * c).max(-1), fr=FR_DIELECTRIC, eta_i=1.0, eta_t=e)
        return out
    if t == abi.MATERIAL_PLASTIC:  # 680-707; Q8: remap_roughness() reads u1.z (674-676), the flag is stored in u0.z (650-655)
        kd, dkd = col(m.u0[0])
        ks, dks = col(m.u0[1])
        ax, ay, dax, day = alphas(m.u0[3], m.u0[3], m.u1[2] != 0)
        return [_lobe(n, LAMBERT, a=kd, da=dkd, present=(kd != 0).any(-1)),
                _lobe(n, MICROFACET, a=ks, da=dks, present=(ks != 0).any(-1), ax=ax, ay=ay, dax=dax, day=day, fr=FR_DIELECTRIC, eta_i=1.5, eta_t=1.0)]
    return []  # None, material.rs:746


def lobe_count(scene, material, uv):
    L = lobes(scene, material, uv)
    return sum(l["present"].astype(np.int64) for l in L) if L else np.zeros(len(uv), np.int64)


# ---- the perturbations of (a), (c), (d) ------------------------------------------------------------------------------------------------------------------
_VEC = {"wo": (BUDGET_XY, BUDGET_XY, BUDGET_Z), "wi": (BUDGET_XY, BUDGET_XY, BUDGET_Z), "wh": (BUDGET_HALF,) * 3, "s_ws": (BUDGET_HALF,) * 3,
        "s_wh": (BUDGET_HALF,) * 3, "s_wi": (BUDGET_REFLECT,) * 3, "s_whe": (BUDGET_HALF,) * 3, "trig": (TRIG_ABS / EPS,) * 2,
        # sample11's scalars that are formed by subtraction move by the roundings of their terms (microfacet.rs:91-98): a = 2 u1 / g1 - 1 by 16 u (1 + |a|)
        # (g1 12 u, the quotient 4 u); the radicand of d by 8 u of its two terms (four products each); slope_x = b tmp -+ d by 4 u of its terms; then
        # slope_x by 8 u and slope_y by 24 u relative (the near branch's root of a quotient; the cubic over the cubic, the root of 1 + slope_x^2, two products)
        # slope_y's cubics are 0.0036 over 0.00049 at u2 = 0 or 1, sums of terms of size 1: each moves by 6 u absolute (three products and three sums, Horner)
        "s11": (16.0, 8.0, 4.0, 8.0, 24.0, 6.0, 6.0)}
# Three more scalars are formed by subtraction from 1 and lose what the vectors' moves do not reach: refract's sin2_t (bxdf.rs:123-124, then 1 - sin2_t:
# 4 u of max(1, eta^2)), fr_dielectric's 1 - cos^2 (2 u) and 1 - sin_t^2 (4 u of max(1, sin_t^2)) (bxdf.rs:150, 157).  One sign each per pattern.
_SCALARS = {"sin2_t": 4.0, "1-c2": 2.0, "1-st2": 4.0}
_NO_SCALAR_MOVES = dict.fromkeys(_SCALARS, 0.0)
_PAR = ("a", "b", "ax", "ay", "eta3", "k3")
_DPAR = {"a": "da", "b": "db", "ax": "dax", "ay": "day", "eta3": "deta", "k3": "dk"}
_SIGNS = np.random.default_rng(20250).choice([-1.0, 1.0], (N_PATTERNS, sum(len(v) for v in _VEC.values()) + len(_PAR) + len(_SCALARS)))


def _pattern(k, n):
    """Pattern k < 0 is no perturbation."""
    P, at = {}, 0
    for name, budget in _VEC.items():
        s = _SIGNS[k, at:at + len(budget)] if k >= 0 else np.zeros(len(budget))
        P[name] = np.broadcast_to(s * np.float64(budget) * EPS, (n, len(budget)))
        at += len(budget)
    P["par"] = dict(zip(_PAR, _SIGNS[k, at:])) if k >= 0 else None
    P["scal"] = {name: _SIGNS[k, at + len(_PAR) + j] * budget * EPS if k >= 0 else 0.0 for j, (name, budget) in enumerate(_SCALARS.items())}
    return P


def _moved(L, par):
    if par is None:
        return L
    out = []
    for l in L:
        l = dict(l)
        for name, s in par.items():
            d = l[_DPAR[name]]
            l[name] = l[name] + s * (d[:, None] if l[name].ndim == 2 else d)
        out.append(l)
    return out


def _in(v):
    """An input as the exact number it is: fp32 unless the caller hands float64 over (the reference's own sampled wi, in the CPU test)."""
    v = np.asarray(v)
    return v if v.dtype == np.float64 else v.astype(np.float32).astype(np.float64)


def _frame(n):
    return onb_from_w(_unit(_in(n)))


def _to_local(onb, a):  # onb.rs:24-26
    return np.stack([_dot(a, onb[0]), _dot(a, onb[1]), _dot(a, onb[2])], -1)


class Result:
    pass


def _aside(allow, ref, flipped):
    a = allow > SET_ASIDE_REL * np.abs(ref) + SET_ASIDE_ABS
    if a.ndim == 2:
        a = a.any(-1)
    return a | flipped | ~np.isfinite(allow if allow.ndim == 1 else allow.max(-1))


def _spread(base, moved):
    """|moved - base| where both are finite; inf where only one is (the caller sets such a sample aside)."""
    with np.errstate(**_IGNORE):
        d = np.abs(moved - base)
    return np.where(np.isfinite(base) & np.isfinite(moved), d, np.where(np.isfinite(base) | np.isfinite(moved), np.inf, 0.0))


# ---- reflection.rs:285-343 -------------------------------------------------------------------------------------------------------------------------------
def _evaluate(L, wo, wi, dwh):
    """Bsdf::f (286-311) and Bsdf::pdf (328-342) on local directions; pdf is 0 for a BSDF without lobes (the probe does not divide by 0)."""
    n = len(wo)
    idx, dec = np.arange(n), Decisions(n)
    f, pdf, count = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int64)
    refl = wi[:, 2] * wo[:, 2] > 0  # dot(wi, ng) dot(wo, ng) > 0 with ng the frame's w
    dec.note("reflect", idx, refl, np.fmin(np.abs(wi[:, 2]), np.abs(wo[:, 2])))
    flat = wo[:, 2] == 0
    dec.note("wo.z==0", idx, flat, np.abs(wo[:, 2]))
    for j, l in enumerate(L):
        count += l["present"]
        k = np.nonzero(l["present"] & refl & ~flat)[0]
        if l["kind"] in _DIFFUSE_REFLECTION and len(k):
            f[k] += LOBE_F[l["kind"]](_sub(l, k), wo[k], wi[k], dwh[k], dec, idx[k], f"f{j}.")
        k = np.nonzero(l["present"])[0]
        if len(k):
            pdf[k] += LOBE_PDF[l["kind"]](_sub(l, k), wo[k], wi[k], dwh[k], dec, idx[k], f"p{j}.")
    with np.errstate(**_IGNORE):
        return f, np.where(count > 0, pdf / count, 0.0), count, dec


def _n_terms(L, table, extra):
    n = len(L[0]["present"]) if L else 0
    return sum(np.where(l["present"], table.get(l["kind"], 0) + extra, 0) for l in L) if L else np.zeros(n)


def evaluate(scene, material, n, uv, wo, wi):
    """f (n, 3), pdf (n,), len (n,) of the material at (n, uv) for world wo, wi; f_allow, pdf_allow; aside["f"], aside["pdf"]; dec."""
    L = lobes(scene, material, uv)
    onb = _frame(n)
    wo_l, wi_l = (_to_local(onb, _in(v)) for v in (wo, wi))
    m = len(wo_l)
    rounds = ~(_axis(onb[0]) & _axis(onb[1]) & _axis(onb[2]))[:, None]
    P = _pattern(-1, m)
    r = Result()
    r.f, r.pdf, r.len, r.dec = _evaluate(L, wo_l, wi_l, Moves(P["wh"], P["scal"]))
    df, dp, flipped = np.zeros((m, 3)), np.zeros(m), np.zeros(m, bool)
    for k in range(N_PATTERNS):
        P = _pattern(k, m)
        f, pdf, _, dec = _evaluate(_moved(L, P["par"]), wo_l + P["wo"] * rounds, wi_l + P["wi"] * rounds, Moves(P["wh"], P["scal"]))
        df, dp = np.fmax(df, _spread(r.f, f)), np.fmax(dp, _spread(r.pdf, pdf))
        flipped |= r.dec.differs(dec)
    flipped |= r.dec.unsafe
    with np.errstate(**_IGNORE):
        r.f_allow = df + EPS * (_n_terms(L, N_F, 1)[:, None] if L else 0) * np.abs(r.f)   # + 1: the sum over the lobes
        r.pdf_allow = dp + EPS * (_n_terms(L, N_PDF, 1) if L else 0) * np.abs(r.pdf)
    r.flipped = flipped
    r.aside = {"f": _aside(r.f_allow, r.f, flipped), "pdf": _aside(r.pdf_allow, r.pdf, flipped)}
    return r


def _sample(L, onb, wo, seeds, P, skip=0):
    """Bsdf::sample_f, reflection.rs:313-326: the lobe by next_u32 % len, the lobe's own sample_f, pdf / len, wi to world."""
    n = len(wo)
    idx, dec, rng = np.arange(n), Decisions(n), Rng(seeds, skip)
    wi, f, pdf = _default(n)
    count = sum(l["present"].astype(np.int64) for l in L) if L else np.zeros(n, np.int64)
    some = np.nonzero(count > 0)[0]
    index = np.full(n, -1, np.int64)
    if len(some):
        index[some] = (rng.u32(some) % count[some].astype(np.uint64)).astype(np.int64)
        dec.note("lobe", some, index[some])
    seen = np.zeros(n, np.int64)
    for j, l in enumerate(L):
        k = np.nonzero(l["present"] & (seen == index))[0]
        seen += l["present"]
        if len(k):
            wi[k], f[k], pdf[k] = LOBE_SAMPLE[l["kind"]](_sub(l, k), wo[k], rng, idx[k], _sub(P, k), dec, f"s{j}.")
    with np.errstate(**_IGNORE):
        pdf = np.where(count > 0, pdf / count, 0.0)
    world = wi[:, 0:1] * onb[0] + wi[:, 1:2] * onb[1] + wi[:, 2:3] * onb[2]  # onb.rs:20-22
    return world, f, pdf, count, index, dec, rng.draws


def sample(scene, material, n, uv, wo, seeds, skip=0):
    """wi (world), f, pdf, len, lobe (the index drawn, -1 without lobes), draws, dec; wi_allow, f_allow, pdf_allow; aside["wi" / "f" / "pdf"].
    skip: how many numbers of PCG32si::new(seed) were drawn before the sample (the integrator's pixel stream: the two jitter draws)."""
    L = lobes(scene, material, uv)
    onb = _frame(n)
    wo_l = _to_local(onb, _in(wo))
    m = len(wo_l)
    rounds = ~(_axis(onb[0]) & _axis(onb[1]) & _axis(onb[2]))[:, None]
    r = Result()
    r.wi, r.f, r.pdf, r.len, r.lobe, r.dec, r.draws = _sample(L, onb, wo_l, seeds, _pattern(-1, m), skip)
    dw, df, dp, flipped = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros(m), np.zeros(m, bool)
    for k in range(N_PATTERNS):
        P = _pattern(k, m)
        wi, f, pdf, _, _, dec, draws = _sample(_moved(L, P["par"]), onb, wo_l + P["wo"] * rounds, seeds, P, skip)
        dw, df, dp = np.fmax(dw, _spread(r.wi, wi)), np.fmax(df, _spread(r.f, f)), np.fmax(dp, _spread(r.pdf, pdf))
        flipped |= r.dec.differs(dec) | (draws != r.draws)
    flipped |= r.dec.unsafe
    kinds = np.full(m, -1)
    seen = np.zeros(m, np.int64)
    for l in L:
        kinds[l["present"] & (seen == r.lobe)] = l["kind"]
        seen += l["present"]
    nf = np.array([N_SAMPLE.get(k, N_F.get(k, 0)) for k in range(-1, 6)])[kinds + 1]
    npdf = np.array([N_SAMPLE.get(k, N_PDF.get(k, 0)) for k in range(-1, 6)])[kinds + 1] + 4  # / len
    with np.errstate(**_IGNORE):
        r.wi_allow = dw + BUDGET_WORLD * EPS
        r.f_allow = df + EPS * nf[:, None] * np.abs(r.f)
        r.pdf_allow = dp + EPS * npdf * np.abs(r.pdf)
    r.flipped = flipped
    r.aside = {"wi": _aside(r.wi_allow, np.ones_like(r.wi), flipped), "f": _aside(r.f_allow, r.f, flipped), "pdf": _aside(r.pdf_allow, r.pdf, flipped)}
    return r


def classes(x):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    x = np.asarray(x, np.float64)
    return np.where(np.isnan(x), 3, np.where(np.isposinf(x), 1, np.where(np.isneginf(x), 2, 0)))


def compare(got, ref, allow, aside):
    """(worst error / allowance over the samples not set aside, the samples that fail).  Where the reference is finite the other side is finite
    and within the allowance; where it is +-inf or NaN the other side has the same class -- also for a sample that is set aside."""
    got, ref, allow = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(allow, np.float64)
    fin = np.isfinite(ref)
    with np.errstate(**_IGNORE):
        err = np.abs(got - ref)
        ratio = np.where(err == 0, 0.0, err / allow)
    held = np.where(fin, np.isfinite(got) & (err <= allow), classes(got) == classes(ref))
    lenient = np.where(fin, np.isfinite(got), classes(got) == classes(ref))  # a set-aside sample still has to have the reference's class
    if got.ndim == 2:
        held, lenient, ratio, fin = held.all(-1), lenient.all(-1), np.where(fin, ratio, 0.0).max(-1), fin.all(-1)
    else:
        ratio = np.where(fin, ratio, 0.0)
    bad = np.where(aside, ~lenient, ~held)
    keep = ~aside & fin
    return (float(ratio[keep].max()) if keep.any() else 0.0), bad


# ---- the scene ---------------------------------------------------------------------------------------------------------------------------------------------
ETA, K = (0.19999069, 0.9220846, 1.0998759), (3.9046354, 2.4476333, 2.1376526)
SINGLE_NON_SPECULAR = ("matte", "matte-checker", "metal-0.25", "metal-0.1", "metal-0.05", "metal-0.01", "metal-aniso", "metal-remap", "metal-clamp",
                       "metal-image", "substrate", "substrate-aniso", "substrate-remap", "substrate-checker", "substrate-image")


class Shared:
    """scene, material[case]."""


@functools.lru_cache(None)
def shared_scene() -> Shared:
    """One quad instance per material.  Every single-lobe kind over Solid textures (resolved at upload into the instance record) and over a
    non-Solid one (the table path, which depends on uv): a Checkerboard kd, ImageMap roughnesses, an ImageMap conductor eta / k."""
    rng = np.random.default_rng(4242)
    s = Scene.new()
    s.set_camera(glam.look_at_lh((0.0, 0.0, -4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), 40.0, 16, 16)
    s.add_texture_image_map(rng.random((3, 3, 3), dtype=np.float32))  # no image under test at offset 0 of the pool
    checker = s.add_texture_checkerboard(s.add_texture_solid((0.7, 0.5, 0.2)), s.add_texture_solid((0.1, 0.3, 0.6)), 5.0, 3.0)
    rough_u = s.add_texture_image_map((0.08 + 0.3 * rng.random((6, 5, 3), dtype=np.float32)).astype(np.float32))
    rough_v = s.add_texture_image_map((0.08 + 0.3 * rng.random((4, 7, 3), dtype=np.float32)).astype(np.float32))
    eta_img = s.add_texture_image_map((0.2 + 1.2 * rng.random((5, 6, 3), dtype=np.float32)).astype(np.float32))
    k_img = s.add_texture_image_map((2.0 + 2.0 * rng.random((7, 4, 3), dtype=np.float32)).astype(np.float32))
    kd, ks, kr, kt = (0.3, 0.25, 0.2), (0.25, 0.3, 0.2), (0.2, 0.15, 0.25), (0.3, 0.3, 0.35)
    zero, half = (0.0, 0.0, 0.0), (0.5, 0.5, 0.5)
    m = {"none": 0}
    m["matte"] = s.add_matte((0.6, 0.4, 0.2))
    m["matte-checker"] = s.add_matte(checker)
    m["glass-1.5"] = s.add_glass(1.5)
    m["glass-1.0001"] = s.add_glass(1.0001)
    m["mirror"] = s.add_mirror((0.9, 0.8, 0.7))
    m["mirror-checker"] = s.add_mirror(checker)
    for a in (0.25, 0.1, 0.05, 0.01):
        m[f"metal-{a}"] = s.add_metal(ETA, K, a, a, remap_roughness=False)
    m["metal-aniso"] = s.add_metal(ETA, K, 0.1, 0.25, remap_roughness=False)
    m["metal-remap"] = s.add_metal(ETA, K, 0.3, 0.1, remap_roughness=True)
    m["metal-clamp"] = s.add_metal(ETA, K, 1e-4, 1e-4, remap_roughness=True)  # below the 1e-3 clamp of roughness_to_alpha
    m["metal-image"] = s.add_metal(eta_img, k_img, rough_u, rough_v, remap_roughness=False)
    m["substrate"] = s.add_substrate((0.5, 0.4, 0.3), (0.2, 0.3, 0.4), 0.1, 0.1, remap_roughness=False)
    m["substrate-aniso"] = s.add_substrate((0.5, 0.4, 0.3), (0.2, 0.3, 0.4), 0.05, 0.25, remap_roughness=False)
    m["substrate-remap"] = s.add_substrate((0.5, 0.4, 0.3), (0.2, 0.3, 0.4), 0.2, 0.4, remap_roughness=True)
    m["substrate-checker"] = s.add_substrate(checker, (0.2, 0.3, 0.4), 0.1, 0.25, remap_roughness=False)
    m["substrate-image"] = s.add_substrate((0.5, 0.4, 0.3), (0.2, 0.3, 0.4), rough_u, rough_v, remap_roughness=True)
    m["plastic"] = s.add_plastic(kd, ks, 0.1)
    m["plastic-nokd"] = s.add_plastic(zero, ks, 0.25)
    m["uber-1"] = s.add_uber(kd, zero, zero, zero)
    m["uber-2"] = s.add_uber(kd, ks, zero, zero, 0.1, 0.2, remap_roughness=False)
    m["uber-3"] = s.add_uber(kd, ks, kr, zero, 0.3, 0.3)
    m["uber-4"] = s.add_uber(kd, ks, kr, kt, 0.1, 0.1, remap_roughness=False)
    m["uber-5"] = s.add_uber(kd, ks, kr, kt, 0.2, 0.1, opacity=half)
    m["uber-opacity0"] = s.add_uber(kd, ks, kr, kt, 0.2, 0.2, opacity=zero)
    m["uber-5-nokd"] = s.add_uber(zero, ks, kr, kt, 0.2, 0.2, opacity=half)
    m["uber-5-noks"] = s.add_uber(kd, zero, kr, kt, 0.2, 0.2, opacity=half)
    m["uber-5-nokr"] = s.add_uber(kd, ks, zero, kt, 0.2, 0.2, opacity=half, eta=1.33)
    m["uber-5-nokt"] = s.add_uber(kd, ks, kr, zero, 0.2, 0.2, opacity=half)
    quad = np.float32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    for k, (case, index) in enumerate(m.items()):
        if index:
            s.add_triangle_mesh(TriangleMesh.from_arrays(quad + np.float32([2.0 * k - 34.0, 0, 0]), np.uint32([0, 1, 2, 0, 2, 3])), index)
    out = Shared()
    out.scene, out.material = s, m
    return out


LOBE_COUNTS = {"none": 0, "matte": 1, "matte-checker": 1, "glass-1.5": 1, "glass-1.0001": 1, "mirror": 1, "mirror-checker": 1, "metal-0.25": 1, "metal-0.1": 1,
               "metal-0.05": 1, "metal-0.01": 1, "metal-aniso": 1, "metal-remap": 1, "metal-clamp": 1, "metal-image": 1, "substrate": 1, "substrate-aniso": 1,
               "substrate-remap": 1, "substrate-checker": 1, "substrate-image": 1, "plastic": 2, "plastic-nokd": 1, "uber-1": 1, "uber-2": 2, "uber-3": 3,
               "uber-4": 4, "uber-5": 5, "uber-opacity0": 3, "uber-5-nokd": 4, "uber-5-noks": 4, "uber-5-nokr": 4, "uber-5-nokt": 4}
CASES = tuple(LOBE_COUNTS)
N_UNIFORM, N_GRAZING = 2048, 1024
SETS = ("uniform", "grazing", "edge")


# ---- the input sets ----------------------------------------------------------------------------------------------------------------------------------------
class Inputs:
    """n, uv, wo, wi (fp32), seeds (uint32), names (the edge rows')."""


def _sphere(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def _pack(n, uv, wo, wi, seeds, names=None):
    out = Inputs()
    out.n, out.uv, out.wo, out.wi = (np.ascontiguousarray(v, np.float32) for v in (n, uv, wo, wi))
    out.seeds, out.names = np.ascontiguousarray(seeds, np.uint32), names
    return out


def _case_rng(case, salt):
    return np.random.default_rng(1000 * salt + CASES.index(case))


def uniform_set(case):
    rng = _case_rng(case, 1)
    return _pack(rng.normal(size=(N_UNIFORM, 3)) * rng.uniform(0.5, 2.0, (N_UNIFORM, 1)), rng.uniform(0, 1, (N_UNIFORM, 2)), _sphere(rng, N_UNIFORM),
                 _sphere(rng, N_UNIFORM), rng.integers(0, 1 << 32, N_UNIFORM, dtype=np.uint64))


# The grazing set's lower end for |cos(wo)| where [2^-20, 2^-3] cannot meet the cap -- the inputs change, not the cap:
#  - a specular lobe's sampled f is colour / |cos(wo)| (bxdf.rs:202, 222, 439-440, 509), and cos(wo) is a dot product with 8 u = 4.8e-7 of absolute
#    error: below |cos| = 80 u = 2^-17.7 the allowance passes 10 % of f.  From 2^-18.5 on, 3.4 % of the set is set aside for it.
#  - Uber's opacity lobe is SpecularTransmission(t, 1, 1) (material.rs:591-593): refract's sin2_t = 1 - cos^2 is within its own roundings of the
#    `>= 1` it is tested against (bxdf.rs:123-128) once cos^2 < 12 u, |cos| < 2^-10.2 -- fp32 rounds 1 - cos^2 to 1 and returns no sample, fp64 does
#    not: ill-conditioning of the specification's own formula, which the set-aside names.  From 2^-11.5 on it stays under the cap.
GRAZING_WO_MIN = {"glass-1.5": -18.5, "glass-1.0001": -18.5, "mirror": -18.5, "mirror-checker": -18.5, "uber-3": -18.5, "uber-4": -15.0,
                  "uber-5": -11.5, "uber-opacity0": -11.5, "uber-5-nokd": -10.5, "uber-5-noks": -10.5, "uber-5-nokr": -10.5, "uber-5-nokt": -11.5}


def grazing_set(case):
    """|cos| log-uniform in [2^-20, 2^-3] (wo: from 2^GRAZING_WO_MIN[case] where that is set), either sign: wo (the first third), wi (the second),
    both (the last)."""
    rng = _case_rng(case, 2)
    n = N_GRAZING
    normals = _sphere(rng, n)
    onb = onb_from_w(_unit(normals.astype(np.float32).astype(np.float64)))

    def around(graze, low):
        z = np.where(graze, 2.0 ** rng.uniform(low, -3, n), rng.uniform(0.15, 1.0, n)) * rng.choice([-1.0, 1.0], n)
        phi = rng.uniform(0, 2 * np.pi, n)
        s = np.sqrt(1 - z * z)
        return (s * np.cos(phi))[:, None] * onb[0] + (s * np.sin(phi))[:, None] * onb[1] + z[:, None] * onb[2]
    third = np.arange(n) * 3 // n
    return _pack(normals, rng.uniform(0, 1, (n, 2)), around(third != 1, GRAZING_WO_MIN.get(case, -20)), around(third != 0, -20), rng.integers(0, 1 << 32, n, dtype=np.uint64))


ALPHAS = (0.25, 0.1, 0.05, 0.01)
G1, G2 = (0.6, 0.0, 0.8), (-0.28, 0.5, 0.8185352772)
SEED = 12345  # an ordinary seed for the rows that are not about the draws


def _tan(t, phi=0.3, below=False):
    c = 1.0 / np.sqrt(1.0 + t * t)
    return (t * c * np.cos(phi), t * c * np.sin(phi), -c if below else c)


@functools.lru_cache(None)
def edge_rows():
    """name -> (n, wo, wi, seed).  With n = +z the frame is u = +y, v = -x exactly, so the local wo, wi are the rows' own numbers (x, y swapped):
    `wo.z == 0` is exact.  Every value is a normal float and none is below 2^-60 unless it is 0."""
    z = (0.0, 0.0, 1.0)
    rows = {}

    def add(name, wo, wi, n=z, seed=SEED):
        rows[name] = (n, wo, wi, seed)
        if n is z:  # the same row below the surface: every relation between wo, wi and n persists
            rows[name + " (below)"] = (n, (wo[0], wo[1], -wo[2]), (wi[0], wi[1], -wi[2]), seed)
    neg = lambda v: tuple(-x for x in v)
    add("wo.z == 0", (1.0, 0.0, 0.0), G1)
    add("wi.z == 0", G1, (0.0, 1.0, 0.0))
    add("wi == -wo", G1, neg(G1))
    add("wi == wo", G1, G1)
    add("wi the mirror of wo", G1, (-0.6, 0.0, 0.8))
    add("wo == n", z, G1)
    add("wo == wi == n", z, z)
    add("wi longer than wo and nearly opposite: dot(wo, wh) < 0", G1, (-2.4, 0.1, 0.25))  # not a unit vector: the only way to a negative dot(wo, wh) in tr_pdf
    for a in ALPHAS:  # wo.z of the stretched wo either side of 0.9999: tan(theta) alpha = tan(acos(0.9999))
        t = np.sqrt(1.0 - 0.9999 ** 2) / 0.9999 / a
        add(f"stretched cos just above 0.9999, alpha {a}", _tan(t * 0.99), G2)  # 1 % in tan: cos_theta 2e-6 either side, far outside the 6 u slack
        add(f"stretched cos just below 0.9999, alpha {a}", _tan(t * 1.01), G2)
        t = 1.0 / (1.6 * a)  # 1 / (alpha |tan|) either side of 1.6
        for what, scale in (("above", 0.999), ("below", 1.001)):
            add(f"a just {what} 1.6 for wo, alpha {a}", _tan(t * scale), G2)
            add(f"a just {what} 1.6 for wi, alpha {a}", G2, _tan(t * scale, phi=2.0))
    for ax, ay in ((0.1, 0.25), (0.05, 0.25)):  # the same after an anisotropic stretch: metal-aniso, substrate-aniso.  Local x = world y, local y = -world x
        for phi in (0.3, 0.8):
            t = np.sqrt(1.0 - 0.9999 ** 2) / 0.9999 / np.sqrt((ax * np.cos(phi)) ** 2 + (ay * np.sin(phi)) ** 2)
            for what, scale in (("above", 0.99), ("below", 1.01)):
                x, y, zz = _tan(t * scale, phi=phi)
                add(f"stretched cos just {what} 0.9999, alphas ({ax}, {ay}), phi {phi}", (-y, x, zz), G2)
    for ir in (1.5, 1.0001, 1.33):  # from inside: at and either side of the critical angle
        sc = 1.0 / ir
        for what, s in (("inside", sc * 0.999), ("at", sc), ("past", min(sc * 1.001, 0.99999))):
            rows[f"from inside, {what} the critical angle of {ir}"] = (z, (s, 0.0, -np.sqrt(1.0 - s * s)), G1, SEED)
    rows["from inside, normal incidence"] = (z, (0.0, 0.0, -1.0), G1, SEED)
    d1, d2 = (0.3, 0.5, 0.8124038), (-0.4, 0.2, 0.8944272)
    for name, n in (("+x", (1, 0, 0)), ("-x", (-1, 0, 0)), ("+y", (0, 1, 0)), ("-y", (0, -1, 0)), ("-z", (0, 0, -1)), ("|n.x| == |n.y|", (0.5, -0.5, 0.7071068)),
                    ("n.x == n.y, z = 0", (1, 1, 0)), ("unnormalised", (0.3, -2.0, 1.5)), ("unnormalised +z", (0, 0, 3))):
        n = tuple(float(v) for v in n)
        add("normal " + name, d1, d2, n=n)
        unit = np.float64(n) / np.linalg.norm(n)
        below = [tuple(float(v) for v in np.float32(np.float64(d) - 2.0 * np.dot(d, unit) * unit)) for d in (d1, d2)]  # mirrored in the surface
        add("normal " + name + " (below)", below[0], below[1], n=n)
    add("first draw below 2^8", G1, G2, seed=seed_with(first=range(0, 256)))
    add("first draw 2^31", G1, G2, seed=seed_with(first=range(1 << 31, (1 << 31) + 64)))
    add("first draw 0xFFFFFFxx", G1, G2, seed=seed_with(first=range(0xFFFFFF00, 1 << 32)))
    add("first next_f32 is 0", G1, G2, seed=seed_with(second=range(0, 256)))
    add("first next_f32 is 1 - 2^-24", G1, G2, seed=seed_with(second=range(0xFFFFFF00, 1 << 32)))
    return rows


# Edge rows whose set-aside is allowed, by the start of their name, with the reason.  Everything else on the edge set has a cap of 0.
_S = ("s_wi", "s_f", "s_pdf")
EDGE_EXEMPT = {  # prefix of the row's name -> (quantities, cases or None for all, reason).  An exemption takes a row out of the cap's count only:
    # check() still compares it, to the allowance wherever the reference's own rule does not set the sample aside
    "wo.z == 0": (_S, None, "a specular lobe's sampled f is colour / |cos(wo)| = colour / 0 (bxdf.rs:202, 439-440): inf, or NaN where the colour's factor is 0 -- "
                  "the class is held; Uber's opacity lobe has sin2_t = 1 exactly, on its threshold (bxdf.rs:126).  Lambert and microfacet lobes are not set aside"),
    "from inside, at the critical angle": (_S, None, "sin2_t >= 1 is decided within an ulp of 1 by construction, for the lobes that refract at that index"),
    "stretched cos just": (_S, ("metal-0.01", "metal-clamp"), "the rows sit 1 % in tan(theta) from sample11's cos_theta > 0.9999 for their own alpha and are held there; "
                           "for these two cases' much smaller alpha the stretched wo is within its roundings of the pole, where cos_phi / sin_phi "
                           "turn the sampled slope about the normal (`sin_theta==0` unsafe), or D's 1 - z^2 takes 10 % of f"),
    "first next_f32 is 0": (_S, None, "where the drawn lobe is a microfacet one it is u1 = 0: a = -1, 1 / (a^2 - 1) is infinite, tmp is the 1e10 cap and slope_x_1 = b tmp - d "
                            "cancels 1e10-fold (microfacet.rs:93-98; `tmp capped` unsafe): fp32 has 0 where fp64 has (1 - b^2) / 2 b.  The class is held; a Lambert or "
                            "specular lobe is not set aside and is held to the allowance"),
}


def edge_exempt(name, quantity, case):
    return any(name.startswith(k) and quantity in q and (cases is None or case in cases) for k, (q, cases, _) in EDGE_EXEMPT.items())


@functools.lru_cache(None)
def edge_set():
    rows = edge_rows()
    names = tuple(rows)
    n, wo, wi, seeds = (np.array([rows[k][j] for k in names], np.float64) for j in range(4))
    uv = np.tile(np.float64([[0.37, 0.61]]), (len(names), 1))
    return _pack(n, uv, wo, wi, seeds.astype(np.uint64), names)


def input_set(case, which):
    return {"uniform": uniform_set, "grazing": grazing_set}[which](case) if which != "edge" else edge_set()


# ---- reference and oracle results, once per (case, set) ----------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def reference(case, which):
    """(Eval, Sample) of the case on the set."""
    S, I = shared_scene(), input_set(case, which)
    m = S.material[case]
    return evaluate(S.scene, m, I.n, I.uv, I.wo, I.wi), sample(S.scene, m, I.n, I.uv, I.wo, I.seeds)


@functools.lru_cache(None)
def oracle_rows(oracle_mod, case, which):
    """(n, 13) from oracle.bsdf_eval: the probe's layout, then the number of random numbers the sample drew."""
    S, I = shared_scene(), input_set(case, which)
    o = _oracle(oracle_mod)
    out = np.zeros((len(I.n), 13), np.float32)
    for i in range(len(I.n)):
        e = o.bsdf_eval(S.material[case], I.n[i], I.uv[i], I.wo[i], I.wi[i], int(I.seeds[i]))
        out[i] = np.concatenate([e["f"], [e["pdf"]], e["s_wi"], e["s_f"], [e["s_pdf"]], [e["len"]], [e["draws"]]])
    return out


@functools.lru_cache(None)
def _oracle(oracle_mod):
    return oracle_mod.Oracle(shared_scene().scene)


QUANTITIES = ("f", "pdf", "s_wi", "s_f", "s_pdf")


def check(rows, case, which):
    """rows (n, 12) in the probe's layout against the reference: {quantity: (worst error / allowance, failing rows)}, and whether len matches.
    A sample is compared by class only where the reference's own rule sets it aside; EDGE_EXEMPT takes a row out of the cap's count, never out of
    this comparison."""
    ev, sm = reference(case, which)
    aside = {"f": ev.aside["f"], "pdf": ev.aside["pdf"], "s_wi": sm.aside["wi"], "s_f": sm.aside["f"], "s_pdf": sm.aside["pdf"]}
    out = {"f": compare(rows[:, 0:3], ev.f, ev.f_allow, aside["f"]), "pdf": compare(rows[:, 3], ev.pdf, ev.pdf_allow, aside["pdf"]),
           "s_wi": compare(rows[:, 4:7], sm.wi, sm.wi_allow, aside["s_wi"]), "s_f": compare(rows[:, 7:10], sm.f, sm.f_allow, aside["s_f"]),
           "s_pdf": compare(rows[:, 10], sm.pdf, sm.pdf_allow, aside["s_pdf"])}
    return out, np.array_equal(rows[:, 11].astype(np.int64), ev.len)


def aside_shares(case, which):
    """{quantity: (share set aside, the rows) }; on the edge set the exempt rows do not count."""
    ev, sm = reference(case, which)
    masks = {"f": ev.aside["f"], "pdf": ev.aside["pdf"], "s_wi": sm.aside["wi"], "s_f": sm.aside["f"], "s_pdf": sm.aside["pdf"]}
    if which == "edge":
        masks = {q: v & ~np.array([edge_exempt(k, q, case) for k in edge_set().names]) for q, v in masks.items()}
    return {k: (float(v.mean()), np.nonzero(v)[0]) for k, v in masks.items()}
