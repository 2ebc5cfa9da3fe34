"""Test helper (not a conftest): the media code of Integrator "volpath" -- Homogeneous::tr / sample / phase / sample_p and the EnumMedium
dispatch -- in numpy and float64, vectorised over samples.  Written from the specification: the reference project's medium.rs:96-158 (180-208
for the vacuum), math.rs:89-97 (coordinate_system), medium.rs:12-21 (spherical_direction) and rand.rs (each function below cites the lines it
follows) -- not from the arithmetic of rene_amd/csrc/device_code.inc and not from oracle/rene_oracle.cpp.  The generator, the decisions'
bookkeeping and the constants (Rng, _unoutput, _unstep, Decisions, EPS, TRIG_ABS, c32) are bsdf_reference's.  Literals are the specification's
fp32 literals (1e-3, pi): a threshold is compared as the fp32 number it is.  Rust's f32::min ignores a NaN operand: np.fmin / np.fmax.

Inputs are exact: the fp32 rd, t_max, wo, wi, sigma_a, sigma_s, g, and the random numbers (integers; next_f32 = (u32 >> 8) 2^-24 is exact).

  evaluate(medium, rd, t_max, wo, wi, seeds) -> Result: tr (n, 3), phase, sampled, position (n, 3), weight (n, 3), p (n, 3), draws, next (the
      stream's next word after the draws: the probe's word 14), per quantity an allowance `allow[q]` and a mask `aside[q]`, `dec` (channel,
      t<t_max, pdf==0, |g|<1e-3, |x|>|y|), `flush` and, for the flush samples, the second admissible answer `alt` (weight, its allowance, aside).

THE ALLOWANCE -- how far an fp32 evaluation of the same specification may lie from this one.  It comes from this reference's own sensitivity
and from operation counts, never from a device's or the oracle's output.  u = 2^-24 (half an fp32 ulp: one correctly rounded operation).
device_math.h states v_rcp_f32, v_rsq_f32, v_sqrt_f32 at 1 ulp (2 u) and qdiv at 2 ulp (4 u).

(a) What fp32 rounds on the way is moved by its counted budget, with N_PATTERNS fixed, seeded sign patterns, and the largest change of the
    fp64 result is taken (MOVES below: each entry with its count):
      len = sqrt(rd.rd): the sum of three squares 3 u relative (positive terms), halved by the root, the root 2 u: 3.5 u -> 4 u relative;
      t = (-ln(1 - u) / sigma_c) / len: two qdiv, 8 u relative, on top of the logarithm's error (b) and len's;
      the exponent sigma_t t len: sigma_a + sigma_s 1 u, two products 2 u: 3 u relative per channel;
      cos_theta = wo.wi: 3 u sum|wo_k wi_k| (exact where either vector is an axis: one product by 0 or +-1, sums with 0);
      denom = 1 + g^2 + 2 g cos: u (g^2 + (1 + g^2) + 2 |g cos| + |denom|) absolute -- against a denom of (1 - |g|)^2 at the peak;
      1 - g^2: u (g^2 + |1 - g^2|) absolute; sample_p's 1 + g - 2 g u0: u (|1 + g| + 2 |g| u0 + |the sum|); sqr_term: qdiv 4 u;
      1 + g^2 - sqr_term^2: u (g^2 + (1 + g^2) + sqr_term^2 + |the sum|) absolute -- divided by 2 g, so at |g| = 1e-3 cos_theta moves by 1e-4;
      cos_theta: qdiv 4 u; 1 - cos_theta^2: u (cos_theta^2 + |1 - cos_theta^2|) absolute;
      the frame of wo (math.rs:89-97; wo is an input): y^2 + z^2 2 u, the root 1 + 2 u, the reciprocal 2 u, the product 1 u: 6 u per component
      of v1, absolute (components <= 1); v2 = wo x v1: products of a moved v1 7 u, the difference 1 u: 8 u; both exact where wo is an axis.
(b) ASSUMED bounds.  v_exp_f32 and v_log_f32 have no bound in device_math.h or in the CDNA guides on hand, so the Vulkan specification's are
    taken, as TRIG_ABS was: exp(x) within (3 + 2 |x|) ulp; log(x) within 3 ulp outside [0.5, 2] and 2^-21 absolute inside.  log(1) = 0 is taken
    as exact (u = 0: -ln(1) = -0, the specification's `-0 / sigma`).  -ln(1 - u) takes its argument in [2^-24, 1], so for u <= 0.5 the absolute
    term rules: LOG_ABS / (sigma_c len) on t -- on `dist`, on `position`, on the weight through the exponent, and it is the slack of `t < t_max`.
    cos(2 pi u1), sin(2 pi u1) carry TRIG_ABS = 2^-11 absolute (bsdf_reference, ASSUMED likewise).
(c) N u |result| for the scalar operations behind them: N_TR = 2 (the exponent's budget is in (a); the negation is free; rounded up), N_PHASE = 10
    (1 / (4 pi) 1, the product 1, the root 2, denom sqrt(denom) 1, qdiv 4 = 9), N_WEIGHT = 10 (density 2, the sum 2, / 3 1, tr sigma_s 1, / pdf
    3 = 9), N_POSITION = 1 (t rd), N_P = 6 absolute (sin_theta's root 2 u and two products, three terms, two sums, of numbers <= 1).
(d) Results below 2^-126.  The device unit is built with denormals flushed and the oracle keeps them; a result under FLT_MIN is therefore 0 or
    a denormal: FLT_MIN absolute on tr, the weight and the position.

THE FLUSH ZONE.  Where the fp64 value of a number the sample passes through -- tr by channel, density by channel, pdf -- lies below
2^-126 (1 + its allowance) the sample is `flush` and has two admissible answers: the IEEE one (denormals kept, quantised to 2^-149, moved by
2^-148 for their roundings; pdf == 0 -> 1 where pdf rounds to 0) and the one with every such number flushed to 0 (pdf == 0 -> 1 included).  A
flush sample passes within the allowance of either.  Flush samples are their own class: they do not count towards the set-aside cap.
For finite inputs pdf itself never gets there: pdf >= density_c / 3 for the channel c that was drawn, and the draw keeps its optical depth
below -ln(2^-24) = 16.6; what flushes is tr, and density, of the *other* channels of a chromatic medium.  `pdf == 0` is therefore recorded
and never taken on these inputs.

SET-ASIDE, bsdf_reference's rule: an allowance beyond 0.1 |reference| + 1e-6 (per channel for tr and the weight; against the vector's length for
position, and against 1 for the unit direction p), or a perturbed evaluation that takes another decision, or a compared number within its own slack
of the threshold.  Caps: 5 % per medium and quantity on the uniform set, 0 on the edge rows apart from EDGE_EXEMPT; asserted from the
reference alone in tests/test_medium_reference.py.

CLASS CHECKS, on every sample (set-aside and flush included): everything finite; tr in [0, 1]; phase >= 0; 0 <= weight <= 3 (1 + 1e-5) per
channel (pdf >= density_c / 3 and sigma_s <= sigma_t: weight_c <= 3 sigma_s / sigma_t, and 3 unsampled); | |p| - 1 | within its allowance;
sampled in {0, 1}; the stream's next word exact; for the vacuum tr = 1, phase = 0, nothing sampled, position 0, weight 1, p = 0, no draw.

The second part is the catalogue the CPU and the GPU test share: one volpath Scene whose media are the cases, and per medium the uniform
set (2 048 rows) and the named edge rows.  The third is the transmittance walks (tr / tr_emit, lib.rs:359-468): walk(), an fp64 restatement over
planes and spheres, its allowance and set-aside rule, and the four walk scenes (slabs, thin, shells, ellipsoid) -- described where it begins."""
import functools

import numpy as np

import bsdf_reference as br
import transform_cases as tc
from bsdf_reference import EPS, TRIG_ABS, Decisions, Rng, _unoutput, _unstep, c32
from rene_amd import abi, glam
from rene_amd.scene import Scene, TriangleMesh

N_PATTERNS = br.N_PATTERNS
SET_ASIDE_REL, SET_ASIDE_ABS, SET_ASIDE_CAP = br.SET_ASIDE_REL, br.SET_ASIDE_ABS, br.SET_ASIDE_CAP
FLT_MIN, DENORM_MIN = 2.0 ** -126, 2.0 ** -149
LOG_ABS, LOG_ULP = 2.0 ** -21, 3.0  # ASSUMED (b): absolute inside [0.5, 2], ulps outside
EXP_ULP = (3.0, 2.0)                # ASSUMED (b): (3 + 2 |x|) ulp
N_TR, N_PHASE, N_WEIGHT, N_POSITION, N_P = 2, 10, 10, 1, 6
WEIGHT_MAX = 3.0 * (1.0 + 1e-5)
PI, G_SWITCH = c32(np.pi), c32(1e-3)
_IGNORE = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")

# (a): name -> how many signs.  The sizes are in _core, next to the number each moves.
MOVES = {"len": 1, "log": 1, "tq": 1, "x": 3, "den": 3, "cos": 1, "denom": 1, "1-g2": 1, "sden": 1, "sqr": 1, "cnum": 1, "cq": 1, "sin": 1, "trig": 2,
         "v1": 3, "v2": 3}
_SIGNS = np.random.default_rng(20251).choice([-1.0, 1.0], (N_PATTERNS, sum(MOVES.values())))


def _pattern(k):
    """Pattern k < 0 is no perturbation."""
    P, at = {}, 0
    for name, count in MOVES.items():
        P[name] = _SIGNS[k, at:at + count] if k >= 0 else np.zeros(count)
        at += count
    return P


class Medium:
    """sigma_a, sigma_s (3,), g as the fp32 numbers the scene holds; vacuum."""

    def __init__(self, sigma_a=(0, 0, 0), sigma_s=(0, 0, 0), g=0.0, vacuum=False):
        self.sigma_a, self.sigma_s = (np.float32(v).astype(np.float64) for v in (sigma_a, sigma_s))
        self.g, self.vacuum = float(np.float32(g)), vacuum


class Result:
    pass


def _in(v):
    return np.asarray(v, np.float32).astype(np.float64)


def _keep(v, mode, sign):
    """A number below FLT_MIN as an fp32 evaluation holds it: "flush" -> 0; "ieee" -> a multiple of 2^-149, moved by 2^-148 for the roundings
    of the operations behind it (0 stays 0 where the value is under a quarter of 2^-149)."""
    small = v < FLT_MIN
    if mode == "flush":
        return np.where(small, 0.0, v)
    q = np.round(v / DENORM_MIN) * DENORM_MIN
    return np.where(small, np.where(v >= DENORM_MIN / 4, np.fmax(q + sign * 2.0 * DENORM_MIN, 0.0), q), v)


def _core(M, rd, t_max, wo, wi, seeds, P, mode):
    """One evaluation under the pattern P; everything float64."""
    n = len(t_max)
    idx, dec, rng = np.arange(n), Decisions(n), Rng(seeds)
    sigma_s, sigma_t, g = M.sigma_s, M.sigma_a + M.sigma_s, M.g  # medium.rs:96-102
    out = Result()
    with np.errstate(**_IGNORE):
        length = np.sqrt((rd * rd).sum(-1)) * (1.0 + P["len"][0] * 4 * EPS)
        # ---- tr, medium.rs:106-108 ----
        out.x_tr = sigma_t * (length * t_max)[:, None] * (1.0 + P["x"] * 3 * EPS)
        out.tr = np.exp(-out.x_tr)
        # ---- sample, medium.rs:110-133 ----
        channel = (rng.u32(idx) % np.uint64(3)).astype(np.int64)                                          # 111
        dec.note("channel", idx, channel)
        u = rng.f32(idx)
        arg = 1.0 - u                                                                                     # exact in fp32: u is a multiple of 2^-24
        L = -np.log(arg) + 0.0
        log_err = np.where(arg == 1.0, 0.0, np.where(arg >= 0.5, LOG_ABS, LOG_ULP * 2 * EPS * np.abs(L)))
        st = sigma_t[channel]
        dist = (L + P["log"][0] * log_err) / st                                                           # 113-114: 0 / 0 = NaN, x / 0 = inf
        t = dist / length * (1.0 + P["tq"][0] * 8 * EPS)                                                  # 115
        sampled = t < t_max                                                                               # 116: false for a NaN
        slack = np.abs(t) * 12 * EPS + log_err / (st * length)
        fin = np.isfinite(t)
        dec.note("t<t_max", idx, sampled, np.where(fin, np.abs(t - t_max), np.inf), np.where(fin, slack, 0.0))
        tt = np.fmin(t, t_max)                                                                            # 117: min ignores the NaN
        out.x = sigma_t * (tt * length)[:, None] * (1.0 + P["x"] * 3 * EPS)                               # 119
        tr_raw = np.exp(-out.x)
        tr = _keep(tr_raw, mode, P["den"])
        dens_raw = np.where(sampled[:, None], sigma_t * tr, tr)                                           # 120
        density = _keep(dens_raw, mode, P["den"])
        pdf_raw = density.sum(-1) / 3.0                                                                   # 121
        pdf = _keep(pdf_raw, mode, P["den"][0])
        zero = pdf == 0.0
        dec.note("pdf==0", idx, zero, pdf, np.where(pdf_raw < FLT_MIN, 2.0 * DENORM_MIN, 0.0))
        pdf = np.where(zero, 1.0, pdf)                                                                    # 122
        out.sampled, out.position = sampled, tt[:, None] * rd                                             # 125-126, ray.origin = 0
        out.weight = np.where(sampled[:, None], tr * sigma_s, tr) / pdf[:, None]                          # 127-131
        out.s_tr, out.s_density, out.s_pdf = tr_raw, dens_raw, pdf_raw
        out.dens_share = density / np.where(density.sum(-1) > 0, density.sum(-1), 1.0)[:, None]
        # ---- phase, medium.rs:135-140 ----
        axis = br._axis(wo) | br._axis(wi)
        cos_theta = (wo * wi).sum(-1) + P["cos"][0] * np.where(axis, 0.0, 3 * EPS * np.abs(wo * wi).sum(-1))
        denom = 1.0 + g * g + 2.0 * g * cos_theta
        denom = denom + P["denom"][0] * EPS * (g * g + (1.0 + g * g) + 2.0 * np.abs(g * cos_theta) + np.abs(denom))
        one_g2 = 1.0 - g * g + P["1-g2"][0] * EPS * (g * g + abs(1.0 - g * g))
        out.phase = 1.0 / (4.0 * PI) * one_g2 / (denom * np.sqrt(denom))
        # ---- sample_p, medium.rs:142-157 ----
        u0, u1 = rng.f32(idx), rng.f32(idx)
        iso = abs(g) < G_SWITCH                                                                           # 146: an exact comparison of an input
        dec.note("|g|<1e-3", idx, np.full(n, iso))
        if iso:
            cos_t = 1.0 - 2.0 * u0                                                                        # 147: exact in fp32
        else:
            sden = 1.0 + g - 2.0 * g * u0
            sden = sden + P["sden"][0] * EPS * (abs(1.0 + g) + 2.0 * abs(g) * u0 + np.abs(sden))
            sqr = one_g2 / sden * (1.0 + P["sqr"][0] * 4 * EPS)                                           # 149
            cnum = 1.0 + g * g - sqr * sqr
            cnum = cnum + P["cnum"][0] * EPS * (g * g + (1.0 + g * g) + sqr * sqr + np.abs(cnum))
            cos_t = -cnum / (2.0 * g) * (1.0 + P["cq"][0] * 4 * EPS)                                      # 150
        s2 = 1.0 - cos_t * cos_t
        sin_t = np.sqrt(np.fmax(s2 + P["sin"][0] * EPS * (cos_t * cos_t + np.abs(s2)), 0.0))              # 153
        phi = 2.0 * PI * u1                                                                               # 154
        first = np.abs(wo[:, 0]) > np.abs(wo[:, 1])                                                       # math.rs:90: a tie takes the second form
        dec.note("|x|>|y|", idx, first, np.abs(np.abs(wo[:, 0]) - np.abs(wo[:, 1])))
        v1, v2, _ = br.onb_from_w(wo)                                                                     # 155; math.rs:89-97
        moves = ~br._axis(wo)[:, None]
        v1, v2 = v1 + moves * P["v1"] * 6 * EPS, v2 + moves * P["v2"] * 8 * EPS
        out.p = ((sin_t * (np.cos(phi) + P["trig"][0] * TRIG_ABS))[:, None] * v1 + (sin_t * (np.sin(phi) + P["trig"][1] * TRIG_ABS))[:, None] * v2
                 + cos_t[:, None] * wo)                                                                   # medium.rs:12-21
        out.cos_t = cos_t
    out.dec, out.draws = dec, rng.draws.copy()
    out.next = br._output(rng.state).astype(np.uint32)
    return out


def _exp_err(x):
    """(b): the relative error of exp(-x), in u."""
    return 2.0 * (EXP_ULP[0] + EXP_ULP[1] * np.abs(x))


def _aside(allow, scale, flipped):
    with np.errstate(**_IGNORE):
        a = ~(allow <= SET_ASIDE_REL * np.abs(scale) + SET_ASIDE_ABS)
    return (a.any(-1) if a.ndim == 2 else a) | flipped


def _vacuum(n, seeds):
    """EnumMedium's dispatch, medium.rs:180-208; SampledMedium::default, 29-37.  No draw."""
    r = Result()
    r.tr, r.phase, r.sampled, r.position, r.weight, r.p = np.ones((n, 3)), np.zeros(n), np.zeros(n, bool), np.zeros((n, 3)), np.ones((n, 3)), np.zeros((n, 3))
    rng = Rng(seeds)
    r.draws, r.next, r.dec = rng.draws.copy(), br._output(rng.state).astype(np.uint32), Decisions(n)
    r.allow = {q: np.zeros_like(np.float64(getattr(r, q))) for q in QUANTITIES}
    r.allow["norm"] = np.zeros(n)
    r.aside = {q: np.zeros(n, bool) for q in QUANTITIES}
    r.flush, r.flipped, r.alt = np.zeros(n, bool), np.zeros(n, bool), None
    return r


QUANTITIES = ("tr", "phase", "position", "weight", "p")


def _variant(M, rd, t_max, wo, wi, seeds, mode):
    base = _core(M, rd, t_max, wo, wi, seeds, _pattern(-1), mode)
    n = len(t_max)
    spread = {q: np.zeros_like(getattr(base, q)) for q in QUANTITIES}
    spread["norm"] = np.zeros(n)
    norm = np.sqrt((base.p * base.p).sum(-1))
    flipped = np.zeros(n, bool)
    for k in range(N_PATTERNS):
        moved = _core(M, rd, t_max, wo, wi, seeds, _pattern(k), mode)
        for q in QUANTITIES:
            spread[q] = np.fmax(spread[q], br._spread(getattr(base, q), getattr(moved, q)))
        spread["norm"] = np.fmax(spread["norm"], br._spread(norm, np.sqrt((moved.p * moved.p).sum(-1))))
        flipped |= base.dec.differs(moved.dec)
    flipped |= base.dec.unsafe
    with np.errstate(**_IGNORE):
        allow = {
            "tr": spread["tr"] + EPS * (N_TR + _exp_err(base.x_tr)) * base.tr + FLT_MIN,
            "phase": spread["phase"] + EPS * N_PHASE * np.abs(base.phase),
            "position": spread["position"] + EPS * N_POSITION * np.abs(base.position) + FLT_MIN,
            # the weight's own exponential, and the exponentials behind pdf by their share of it
            "weight": spread["weight"] + EPS * (N_WEIGHT + _exp_err(base.x) + (base.dens_share * _exp_err(base.x)).sum(-1)[:, None]) * np.abs(base.weight) + FLT_MIN,
            "p": spread["p"] + EPS * N_P,
            "norm": spread["norm"] + 2 * EPS * N_P + np.abs(norm - 1.0),
        }
    base.allow, base.flipped, base.norm = allow, flipped, norm
    length = np.sqrt((base.position * base.position).sum(-1))[:, None]
    base.aside = {"tr": _aside(allow["tr"], base.tr, np.zeros(n, bool)), "phase": _aside(allow["phase"], base.phase, np.zeros(n, bool)),
                  "position": _aside(allow["position"], length, flipped), "weight": _aside(allow["weight"], base.weight, flipped),
                  "p": _aside(allow["p"], np.ones_like(base.p), flipped)}
    return base


def evaluate(medium, rd, t_max, wo, wi, seeds):
    rd, t_max, wo, wi = _in(rd), _in(t_max), _in(wo), _in(wi)
    seeds = np.asarray(seeds).astype(np.uint64)
    if medium.vacuum:
        return _vacuum(len(t_max), seeds)
    r = _variant(medium, rd, t_max, wo, wi, seeds, "ieee")
    # the flush zone: a number the sample passes through, below FLT_MIN (1 + its allowance); the allowance of such a number is its exponent's
    # (|x| times the 15 u of t, len and the products, rounded up to 20) and the exponential's own
    rel = EPS * (20.0 * np.abs(r.x) + _exp_err(r.x) + N_WEIGHT)
    zone = lambda v, a: (v >= DENORM_MIN / 4) & (v < FLT_MIN * (1 + a))  # under a quarter of 2^-149 both answers are 0, as for an exact 0 (sigma_t = 0)
    r.flush = (zone(r.s_tr, rel) | zone(r.s_density, rel)).any(-1) | zone(r.s_pdf, rel.max(-1))
    r.alt = _variant(medium, rd, t_max, wo, wi, seeds, "flush") if r.flush.any() else None
    return r


# ---- seeds for one chosen draw -----------------------------------------------------------------------------------------------------------------------------
def draws_of(seed, count):
    r, one = Rng([seed]), np.array([0])
    return [int(r.u32(one)[0]) for _ in range(count)]


def seed_with_draw(k, candidates, also=None):
    """A seed whose k-th next_u32 (k = 1 the first) is the first of `candidates` that has one: the output permutation and k - 1 steps of the LCG are
    inverted; new() maps a seed to step(seed (MUL + 1) + INC) and MUL + 1 is even, so only every other state has a seed.  also(draws) filters
    on the first k draws: a second property comes from filtering the candidates of the first."""
    for t in candidates:
        s0 = _unoutput(t)
        for _ in range(k - 1):
            s0 = _unstep(s0)
        r = (_unstep(s0) - br._INC) & br.M32
        if r % 2:
            continue
        seed = (r // 2 * pow((br._MUL + 1) // 2, -1, 1 << 31)) % (1 << 31)
        d = draws_of(seed, k)
        assert d[k - 1] == t
        if also is None or also(d):
            return seed
    raise ValueError("no seed")


# ---- the catalogue -------------------------------------------------------------------------------------------------------------------------------------------
_G3 = float(np.float32(1e-3))
G_VALUES = (0.0, 0.3, -0.3, 0.7, -0.7, 0.9, -0.9, 0.99, -0.99, 0.999, -0.999) + tuple(
    s * v for v in (float(np.nextafter(np.float32(1e-3), np.float32(0))), _G3, 1.001e-3) for s in (1.0, -1.0))
SIGMAS = {  # name -> (sigma_a, sigma_s)
    "grey": ((0.25, 0.25, 0.25), (0.75, 0.75, 0.75)),                # sigma_t = (1, 1, 1)
    "chromatic": ((0.02, 0.4, 8.0), (0.03, 0.6, 12.0)),             # sigma_t = (0.05, 1, 20)
    "one channel empty": ((0.3, 0.0, 0.5), (0.7, 0.0, 1.5)),        # sigma_a = sigma_s = 0 in g: rcp(0), -0 inf
    "sigma_s = 0": ((0.3, 0.7, 1.3), (0.0, 0.0, 0.0)),
    "sigma_a = 0": ((0.0, 0.0, 0.0), (0.5, 1.0, 2.0)),
    "thin": ((0.4e-6, 0.4e-6, 0.4e-6), (0.6e-6, 0.6e-6, 0.6e-6)),  # sigma_t = 1e-6
    "dense": ((10.0, 20.0, 30.0), (30.0, 40.0, 60.0)),               # sigma_t = (40, 60, 90): t_max <= 3 crosses both ends of the flush zone
    "defaults": ((0.0011, 0.0024, 0.014), (2.55, 3.21, 3.77)),       # the loader's, intermediate_scene.rs:896-904
}


def _media():
    out = {"vacuum": None}
    for g in G_VALUES:
        out[f"grey g={g!r}"] = SIGMAS["grey"] + (g,)
    for name, s in SIGMAS.items():
        if name != "grey":
            out[f"{name} g=0.0"] = s + (0.0,)
            out[f"{name} g=0.7"] = s + (0.7,)
    out["dense g=-0.99"] = SIGMAS["dense"] + (-0.99,)
    return out


MEDIA = _media()
CASES = tuple(MEDIA)
N_UNIFORM = 2048
SETS = ("uniform", "edge")


def medium_of(case) -> Medium:
    m = MEDIA[case]
    return Medium(vacuum=True) if m is None else Medium(*m)


class Shared:
    """scene, index[case]."""


@functools.lru_cache(None)
def shared_scene() -> Shared:
    """One volpath Scene whose media are the cases (medium 0 is the scene's vacuum); one Matte quad so that there is something to pack."""
    s = Scene.new()
    s.integrator = abi.INTEGRATOR_VOLPATH
    s.set_camera(glam.look_at_lh((0.0, 0.0, -4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), 40.0, 16, 16)
    index = {"vacuum": 0}
    for case, m in MEDIA.items():
        if m is not None:
            index[case] = s.add_medium_homogeneous(*m)
    quad = np.float32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    s.add_triangle_mesh(TriangleMesh.from_arrays(quad, np.uint32([0, 1, 2, 0, 2, 3])), s.add_matte((0.5, 0.5, 0.5)))
    out = Shared()
    out.scene, out.index = s, index
    return out


class Inputs:
    """rd, wo, wi (n, 3), t_max (n,) fp32, seeds uint32, names (the edge rows')."""


def _pack(rd, t_max, wo, wi, seeds, names=None):
    out = Inputs()
    out.rd, out.t_max, out.wo, out.wi = (np.ascontiguousarray(v, np.float32) for v in (rd, t_max, wo, wi))
    out.seeds, out.names = np.ascontiguousarray(np.asarray(seeds).astype(np.uint64), np.uint32), names
    return out


def uniform_set(case):
    """rd on the sphere times [2^-3, 2^3] log-uniform, t_max log-uniform in [2^-6, 2^3], wo and wi uniform on the sphere, random seeds."""
    rng = np.random.default_rng(7000 + CASES.index(case))
    n = N_UNIFORM
    return _pack(br._sphere(rng, n) * 2.0 ** rng.uniform(-3, 3, (n, 1)), 2.0 ** rng.uniform(-6, 3, n), br._sphere(rng, n), br._sphere(rng, n),
                 rng.integers(0, 1 << 32, n, dtype=np.uint64))


RD, WO, WI, ROW_T_MAX, SEED = (0.3, -0.5, 0.8124038), (0.6, 0.0, 0.8), (-0.28, 0.5, 0.8185352772), 0.7, 12345
AXES = {"+x": (1.0, 0.0, 0.0), "-x": (-1.0, 0.0, 0.0), "+y": (0.0, 1.0, 0.0), "-y": (0.0, -1.0, 0.0), "+z": (0.0, 0.0, 1.0), "-z": (0.0, 0.0, -1.0)}
TAUS = (87.0, 87.7, 103.6, 104.4, 200.0)  # either side of 87.34 (2^-126) and of 103.97 (2^-149), and far beyond
_TOP = 0xFFFFFF00


@functools.lru_cache(None)
def _edge_seeds():
    out = {}
    for c in range(3):  # the distance draw (the second) with each channel (the first draw % 3): 256 candidates, half have a seed
        out[f"distance draw 0, channel {c}"] = seed_with_draw(2, range(0, 256), lambda d, c=c: d[0] % 3 == c)
        out[f"distance draw 1 - 2^-24, channel {c}"] = seed_with_draw(2, range(_TOP, 1 << 32), lambda d, c=c: d[0] % 3 == c)
    out["channel draw 0xFFFFFFFF"] = seed_with_draw(1, range(0xFFFFFFFF, _TOP, -1))  # the largest word that has a seed
    out["u0 = 0"] = seed_with_draw(3, range(0, 256))
    out["u0 = 1 - 2^-24"] = seed_with_draw(3, range(_TOP, 1 << 32))
    for name, q in (("0", 0), ("1/4", 1 << 30), ("1/2", 1 << 31), ("3/4", 3 << 30)):
        out[f"u1 = {name}"] = seed_with_draw(4, range(q, q + 256))
    return out


@functools.lru_cache(None)
def edge_rows(case):
    """name -> (rd, t_max, wo, wi, seed).  The optical-depth rows depend on the medium: t_max = tau / (the largest sigma_t) along rd = +z."""
    rows = {}

    def add(name, rd=RD, t_max=ROW_T_MAX, wo=WO, wi=WI, seed=SEED):
        rows[name] = (rd, t_max, wo, wi, seed)
    neg = lambda v: tuple(-x for x in v)
    add("t_max = 0", t_max=0.0)
    add("|rd| = 2^-10", rd=tuple(x * 2.0 ** -10 for x in RD))
    add("|rd| = 2^10", rd=tuple(x * 2.0 ** 10 for x in RD))
    m = MEDIA[case]
    top = 1.0 if m is None else float(np.float32(np.float32(m[0]) + np.float32(m[1])).max())
    for tau in TAUS:
        add(f"optical depth {tau} in the densest channel", rd=AXES["+z"], t_max=tau / top)
    for name, seed in _edge_seeds().items():
        add(name, seed=seed)
    for name, a in AXES.items():
        add(f"wo = {name}", wo=a)
        if name[0] == "+":
            add(f"wi = wo = {name}", wo=a, wi=a)
            add(f"wi = -wo, wo = {name}", wo=a, wi=neg(a))
    perp = np.float64([0.8, 0.0, -0.6])
    for e in (-10, -20):
        wi = np.cos(2.0 ** e) * np.float64(WO) + np.sin(2.0 ** e) * perp
        add(f"wi 2^{e} rad from wo", wi=tuple(wi))
        add(f"wi 2^{e} rad from -wo", wi=tuple(-wi))
    add("|wo.x| == |wo.y|", wo=(0.5, -0.5, 0.7071068))
    return rows


# Edge rows whose set-aside is allowed: the start of the row's name -> (quantities, the cases, the reason).  Everything else has a cap of 0.
_PEAK = ("at |g| = 0.999 the peak's denom is (1 - |g|)^2 = 1e-6 and 1 + g^2 + 2 g cos carries 5 u = 3e-7 of roundings (8 u off an axis), each "
         "worth 1.5 times its share of the phase: beyond 10 %.  Held by class (finite, >= 0); the rows of |g| = 0.99, whose peak is 1e-4, are held to the allowance")
EDGE_EXEMPT = {
    "wi = -wo": (("phase",), ("grey g=0.999",), _PEAK),
    "wi 2^-10 rad from -wo": (("phase",), ("grey g=0.999",), _PEAK),
    "wi 2^-20 rad from -wo": (("phase",), ("grey g=0.999",), _PEAK),
    "wi = wo": (("phase",), ("grey g=-0.999",), _PEAK),
    "wi 2^-10 rad from wo": (("phase",), ("grey g=-0.999",), _PEAK),
    "wi 2^-20 rad from wo": (("phase",), ("grey g=-0.999",), _PEAK),
}


def edge_exempt(name, quantity, case):
    return any(name.startswith(k) and quantity in q and case in cases for k, (q, cases, _) in EDGE_EXEMPT.items())


@functools.lru_cache(None)
def edge_set(case):
    rows = edge_rows(case)
    names = tuple(rows)
    rd, wo, wi = (np.array([rows[k][j] for k in names], np.float64) for j in (0, 2, 3))
    return _pack(rd, np.array([rows[k][1] for k in names]), wo, wi, np.array([rows[k][4] for k in names], np.uint64), names)


def input_set(case, which):
    return uniform_set(case) if which == "uniform" else edge_set(case)


@functools.lru_cache(None)
def reference(case, which):
    I = input_set(case, which)
    return evaluate(medium_of(case), I.rd, I.t_max, I.wo, I.wi, I.seeds)


@functools.lru_cache(None)
def oracle_rows(oracle_mod, case, which):
    """(n, 16) from oracle.medium_eval: the probe's layout."""
    S, I = shared_scene(), input_set(case, which)
    o = oracle_mod.Oracle(S.scene)  # a scene of one quad: made and closed per call, nothing is left for the interpreter's exit
    try:
        return o.medium_eval(S.index[case], I.rd, I.t_max, I.wo, I.wi, I.seeds)
    finally:
        o.close()


# ---- the comparison ------------------------------------------------------------------------------------------------------------------------------------------
def _ratio(got, ref, allow):
    """error / allowance per sample (the largest over a vector's components); inf where the probe's number is not finite."""
    with np.errstate(**_IGNORE):
        err = np.abs(np.asarray(got, np.float64) - ref)
        r = np.where(err == 0, 0.0, err / allow)
    r = np.where(np.isfinite(got), r, np.inf)
    return r.max(-1) if r.ndim == 2 else r


_COLS = {"tr": slice(0, 3), "phase": 3, "position": slice(5, 8), "weight": slice(8, 11), "p": slice(11, 14)}


def check(rows, case, which):
    """rows (n, 16) in the layout of rene_medium_eval against the reference.  Returns
      result: {quantity: (worst error / allowance over the samples not set aside, the failing samples)} -- a sample that the reference's own
              rule sets aside is held by class only; a flush sample passes within the allowance of either admissible answer;
      classes: {name: failing samples} for the class checks, which hold on every sample;
      flush: {"rows", "ieee", "flushed", "both"}: how many flush samples there are and which answer the weight sits on."""
    ref = reference(case, which)
    rows = np.asarray(rows, np.float32)
    n = len(rows)
    result, flush = {}, {"rows": int(ref.flush.sum()), "ieee": 0, "flushed": 0, "both": 0}
    for q in QUANTITIES:
        got = rows[:, _COLS[q]].astype(np.float64)
        finite = np.isfinite(got).all(-1) if got.ndim == 2 else np.isfinite(got)
        ratio, aside = _ratio(got, getattr(ref, q), ref.allow[q]), ref.aside[q]
        ok = np.where(aside, finite, ratio <= 1.0)
        if ref.alt is not None:
            r2, a2 = _ratio(got, getattr(ref.alt, q), ref.alt.allow[q]), ref.alt.aside[q]
            ok2 = ref.flush & np.where(a2, finite, r2 <= 1.0)
            if q == "weight":
                on1, on2 = ref.flush & ~aside & (ratio <= 1.0), ref.flush & ~a2 & (r2 <= 1.0)
                flush.update(ieee=int((on1 & ~on2).sum()), flushed=int((on2 & ~on1).sum()), both=int((on1 & on2).sum()))
            ratio = np.where(ref.flush & ~a2, np.where(aside, r2, np.fmin(ratio, r2)), ratio)
            aside, ok = np.where(ref.flush, aside & a2, aside), ok | ok2
        keep = ~aside
        result[q] = (float(ratio[keep].max()) if keep.any() else 0.0, ~ok)
    tr, phase, w, p = rows[:, 0:3], rows[:, 3], rows[:, 8:11], rows[:, 11:14].astype(np.float64)
    classes = {
        "finite": ~np.isfinite(rows[:, :14]).all(-1),
        "tr in [0, 1]": ~((tr >= 0) & (tr <= 1)).all(-1),
        "phase >= 0": ~(phase >= 0),
        "0 <= weight <= 3": ~((w >= 0) & (w <= np.float32(WEIGHT_MAX))).all(-1),
        "sampled in {0, 1}": ~np.isin(rows[:, 4], (0.0, 1.0)),
        "sampled": (rows[:, 4] != ref.sampled) & ~ref.flipped,
        "next word": rows[:, 14].view(np.uint32) != ref.next,
    }
    if medium_of(case).vacuum:
        classes["vacuum"] = ~((tr == 1).all(-1) & (rows[:, 3:8] == 0).all(-1) & (w == 1).all(-1) & (p == 0).all(-1))
        classes["draws"] = ref.draws != 0
    else:
        with np.errstate(**_IGNORE):
            classes["|p| = 1"] = ~(np.abs(np.sqrt((p * p).sum(-1)) - 1.0) <= ref.allow["norm"])
        classes["draws"] = ref.draws != 4  # sample: the channel and the distance; sample_p: u0 and u1
    return result, classes, flush


def oracle_flush_on_ieee(rows, case, which):
    """The oracle keeps denormals: its flush samples sit on the IEEE answer.  The samples that do not."""
    ref = reference(case, which)
    got = np.asarray(rows, np.float32)[:, _COLS["weight"]].astype(np.float64)
    return ref.flush & ~ref.aside["weight"] & ~(_ratio(got, ref.weight, ref.allow["weight"]) <= 1.0)


def aside_shares(case, which):
    """{quantity: (share set aside, the rows)}: flush samples are their own class and do not count; on the edge rows the exempt ones do not either."""
    ref = reference(case, which)
    masks = {q: ref.aside[q] & ~ref.flush for q in QUANTITIES}
    if which == "edge":
        names = edge_set(case).names
        masks = {q: v & ~np.array([edge_exempt(k, q, case) for k in names]) for q, v in masks.items()}
    return {q: (float(v.mean()), np.nonzero(v)[0]) for q, v in masks.items()}


# =============================================================================================================================================================
# The transmittance walks, tr / tr_emit, lib.rs:359-468, over analytic geometry: rectangles in planes z = const and spheres under an affine map.
#
#   walk(description, emit, medium, ro, rd) -> Result: tr (n, 3), queries (n,), allow (n, 3), aside (n,), ended (n,): how the walk ended
#
# The loop of lib.rs:371-408 / 425-467: the next surface with 0.001 < t <= 1e5 in units of |rd| (a miss: tr, or 0 for tr_emit: 391-392, 445-446);
# tr_emit's area light first -- tr times its radiance where dot(-normalize(rd), n) > 0, else 0 (447-451; area_light.rs's emit) --; a material that
# is not None blocks (393-394, 452-453); otherwise tr *= exp(-sigma_t |rd| t) unless the medium is the vacuum (396-399, medium.rs:106-108), the
# medium becomes the surface's exterior where dot(rd, n) > 0 and its interior otherwise (401-405), with n the SHADING normal the closest-hit
# shader returns (the vertex normals of a mesh, lib.rs:931-951; M^-T p of a sphere, 874-880), and the ray restarts at the hit position (406).
# Three quirks follow and are pinned: a boundary within 0.001 |rd| behind another is skipped (the restart's tmin); a mesh whose vertex normals
# point the other way than its interior / exterior were meant switches to the "wrong" medium; and the segment that ends on tr_emit's area light
# carries no factor (447-451 return before 455-458 multiply), nor does the one that ends on a blocker or on nothing.
#
# The allowance: each crossing's t moves by transform_cases.margin(t), what that module grants rene_trace, through sigma_t |rd| dt; plus, per
# crossing, the exponent's 3 u (a), the ASSUMED exp bound (b) and the product's 1 u; plus 1 u for tr_emit's product; FLT_MIN absolute (d).
# Set aside, from the reference alone: a ray for which a perturbed walk would cross another number of surfaces or meet another terminator --
# a candidate t within twice the margin of 0.001 |rd|-units or of another candidate's (a tie), a hit within transform_cases.EDGE of a rectangle's
# rim or diagonal (in the rectangle's own coordinates), a sphere met with disc / half_b^2 < GRAZING_DISC or with its roots within ROOT_GAP, a
# cosine between the ray and the normal below PARALLEL where the normal's side decides (the switch, the emitter's facing test); and the usual
# 0.1 |reference| + 1e-6.  At most 5 % per scene and start medium, apart from WALK_EXEMPT.
# =============================================================================================================================================================
T_MIN, T_MAX, MAX_CROSSINGS = c32(0.001), c32(1e5), 64
ENDED = ("miss", "blocked", "emitter facing", "emitter averted")


class Rect:
    """A rectangle [x0, x1] x [y0, y1] in the plane z, as two triangles with the vertex normals (0, 0, nz)."""

    def __init__(self, z, x, y, nz, material="none", emit=None, interior=0, exterior=0):
        self.z, self.x, self.y = float(np.float32(z)), tuple(float(np.float32(v)) for v in x), tuple(float(np.float32(v)) for v in y)
        self.nz, self.material, self.emit, self.interior, self.exterior = float(nz), material, emit, interior, exterior

    def hit(self, o, d):
        """t (NaN for a miss), the shading normal, near: within EDGE of the rim or of the diagonal the two triangles share."""
        with np.errstate(**_IGNORE):
            t = (self.z - o[:, 2]) / d[:, 2]
            p = o + t[:, None] * d
            u, v = (p[:, 0] - self.x[0]) / (self.x[1] - self.x[0]), (p[:, 1] - self.y[0]) / (self.y[1] - self.y[0])
            inside = (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1)
            edge = np.fmin(np.fmin(np.fmin(np.abs(u), np.abs(1 - u)), np.fmin(np.abs(v), np.abs(1 - v))), np.abs(u - v))
        t = np.where(inside & np.isfinite(t), t, np.nan)
        near = np.isfinite(t) & (edge < tc.EDGE) | (~inside & (edge < tc.EDGE) & (u > -tc.EDGE) & (u < 1 + tc.EDGE) & (v > -tc.EDGE) & (v < 1 + tc.EDGE))
        return t, np.tile(np.float64([[0.0, 0.0, self.nz]]), (len(o), 1)), near


class Ball:
    """The unit sphere under the 4 x 4 map m (fp32 entries); its normal points outwards."""

    def __init__(self, m, material="none", emit=None, interior=0, exterior=0):
        self.m = np.asarray(m, np.float32).astype(np.float64)
        self.material, self.emit, self.interior, self.exterior = material, emit, interior, exterior

    def hit(self, o, d):
        t, normal, disc_n, roots = tc.ray_sphere(self.m, o, d, tmin=-np.inf, tmax=np.inf)
        with np.errstate(**_IGNORE):
            ok = (roots > T_MIN) & (roots <= T_MAX)
            t = np.where(ok[:, 0], roots[:, 0], np.where(ok[:, 1], roots[:, 1], np.nan))
            inv = np.linalg.inv(self.m[:3, :3])
            p = (o - self.m[:3, 3]) @ inv.T + np.nan_to_num(t)[:, None] * (d @ inv.T)
            near = (np.abs(disc_n) < tc.GRAZING_DISC) | ((roots[:, 1] - roots[:, 0] < tc.ROOT_GAP) & (roots[:, 1] > -tc.ROOT_GAP))
            near |= (np.abs(roots - T_MIN) < 2 * tc.margin(T_MIN)).any(-1)
        return t, p @ inv, near & np.isfinite(disc_n)


class Description:
    """media: [None (the vacuum), (sigma_a, sigma_s, g), ...]; surfaces: Rect / Ball."""

    def __init__(self, media, surfaces):
        self.media, self.surfaces = media, surfaces
        self.sigma_t = [None if m is None else (np.float32(m[0]) + np.float32(m[1])).astype(np.float64) for m in media]


def walk(description, emit, medium, ro, rd):
    ro, rd = _in(ro).copy(), _in(rd)
    n = len(ro)
    length = np.sqrt((rd * rd).sum(-1))
    medium = np.full(n, medium, np.int64)
    r = Result()
    r.tr, r.queries, r.ended, r.aside = np.ones((n, 3)), np.zeros(n, np.int64), np.full(n, -1), np.zeros(n, bool)
    rel = np.zeros((n, 3))
    live = np.ones(n, bool)
    S = description.surfaces
    for _ in range(MAX_CROSSINGS):
        if not live.any():
            break
        r.queries += live
        hits = [s.hit(ro, rd) for s in S]
        with np.errstate(**_IGNORE):
            ts = np.stack([np.where((t > T_MIN) & (t <= T_MAX), t, np.inf) for t, _, _ in hits], -1)
            raw = np.stack([np.where(np.isfinite(t), t, np.inf) for t, _, _ in hits], -1)
            order = np.argsort(ts, -1)
            first = order[:, 0]
            t = np.take_along_axis(ts, order[:, :1], -1)[:, 0]
            second = np.take_along_axis(ts, order[:, 1:2], -1)[:, 0] if len(S) > 1 else np.full(n, np.inf)
            m2 = 2 * tc.margin(np.where(np.isfinite(t), t, 0.0))
            doubt = np.isfinite(t) & (second - t < m2)                                                    # a tie
            doubt |= (np.abs(raw - T_MIN) < 2 * tc.margin(T_MIN)).any(-1)                                 # a candidate on the restart's tmin
            doubt |= np.stack([near for _, _, near in hits], -1).any(-1)                                  # a rim, a diagonal or a limb, hit or just missed
        miss = live & ~np.isfinite(t)
        r.ended[miss] = 0
        if emit:
            r.tr[miss] = 0.0                                                                              # lib.rs:445-446
        r.aside |= live & doubt
        live = live & ~miss
        for k, s in enumerate(S):
            here = live & (first == k)
            if not here.any():
                continue
            normal = hits[k][1]
            with np.errstate(**_IGNORE):
                cos = (rd * normal).sum(-1) / (length * np.sqrt((normal * normal).sum(-1)))
            if emit and s.emit is not None:                                                               # 447-451
                facing = -cos > 0
                r.aside |= here & (np.abs(cos) < tc.PARALLEL)
                r.tr[here] = np.where(facing[here, None], r.tr[here] * np.float32(s.emit).astype(np.float64), 0.0)
                rel[here] += EPS
                r.ended[here] = np.where(facing[here], 2, 3)
                live = live & ~here
            elif s.material != "none":                                                                    # 393-394, 452-453
                r.tr[here], r.ended[here] = 0.0, 1
                live = live & ~here
            else:
                for mi in np.unique(medium[here]):
                    st = description.sigma_t[mi]
                    if st is None:                                                                        # 396-399
                        continue
                    w = here & (medium == mi)
                    x = st * (length[w] * t[w])[:, None]                                                  # medium.rs:106-108
                    r.tr[w] *= np.exp(-x)
                    rel[w] += st * (length[w] * tc.margin(t[w]))[:, None] + EPS * (3 * x + _exp_err(x) + 1)
                r.aside |= here & (np.abs(cos) < tc.PARALLEL)
                medium = np.where(here, np.where(cos > 0, s.exterior, s.interior), medium)               # 401-405
                ro = np.where(here[:, None], ro + t[:, None] * rd, ro)                                    # 406
    assert not live.any(), "a walk did not end"
    r.allow = r.tr * rel + FLT_MIN
    with np.errstate(**_IGNORE):
        r.aside |= ~(r.allow <= SET_ASIDE_REL * np.abs(r.tr) + SET_ASIDE_ABS).all(-1)
    return r


# ---- the walk scenes ---------------------------------------------------------------------------------------------------------------------------------------------
_CHROMA1, _CHROMA2 = ((0.02, 0.1, 0.3), (0.08, 0.3, 0.9)), ((0.5, 0.1, 0.02), (0.7, 0.2, 0.05))
_GREY1, _GREY2 = ((0.1, 0.1, 0.1), (0.3, 0.3, 0.3)), ((0.05, 0.05, 0.05), (0.15, 0.15, 0.15))
_L = (2.0, 3.0, 4.0)
_BIG = (-60.0, 60.0)
N_WALK = 1024


def _slabs():
    """Five None rectangles at z = 1 .. 5 with media 1 (chromatic), 2 (chromatic), the vacuum and 3 between them, medium 4 behind.  The one at z = 2
    has its vertex normals flipped and its interior / exterior swapped to match; the one at z = 4 has them flipped and nothing swapped, so the
    walk carries the vacuum on through [4, 5] where medium 3 was meant: the quirk, pinned.  At z = 6, by x: nothing (x < -10), a Matte wall
    [-10, 0], an emitter facing the rays [0, 10], an emitter averted [10, 20]."""
    media = [None, _CHROMA1 + (0.0,), _CHROMA2 + (0.3,), _GREY1 + (0.0,), _GREY2 + (0.0,)]
    return Description(media, [
        Rect(1, _BIG, _BIG, -1, interior=1, exterior=0),
        Rect(2, _BIG, _BIG, +1, interior=1, exterior=2),
        Rect(3, _BIG, _BIG, -1, interior=0, exterior=2),
        Rect(4, _BIG, _BIG, +1, interior=3, exterior=0),
        Rect(5, _BIG, _BIG, -1, interior=4, exterior=3),
        Rect(6, (-10, 0), _BIG, -1, material="matte"),
        Rect(6, (0, 10), _BIG, -1, material="matte", emit=_L),
        Rect(6, (10, 20), _BIG, +1, material="matte", emit=_L)])


def _slabs_rays(rng, n):
    """0 to 80 degrees from the axis, |rd| in {0.5, 1, 2}, aimed at (x in [-19.5, 19.5], y in [-2, 2]) of the plane z = 6 from z = 0."""
    theta, phi = np.radians(rng.uniform(0, 80, n)), rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], -1)
    target = np.stack([rng.uniform(-19.5, 19.5, n), rng.uniform(-2, 2, n), np.full(n, 6.0)], -1)
    return target - d * (6.0 / d[:, 2])[:, None], d * rng.choice([0.5, 1.0, 2.0], n)[:, None]


def _thin():
    """Pairs of boundaries 0.0005 and 0.002 apart.  The second of a pair is skipped exactly when it lies within 0.001 |rd|-units of the first: the
    medium then lasts to the next boundary.  An emitter at z = 3 faces the rays."""
    media = [None, _CHROMA1 + (0.0,), _CHROMA2 + (0.0,)]
    return Description(media, [
        Rect(1, _BIG, _BIG, -1, interior=1, exterior=0), Rect(1.0005, _BIG, _BIG, -1, interior=0, exterior=1),
        Rect(2, _BIG, _BIG, -1, interior=2, exterior=0), Rect(2.002, _BIG, _BIG, -1, interior=0, exterior=2),
        Rect(3, _BIG, _BIG, -1, material="matte", emit=_L)])


THIN_LENGTHS = (1.0, 1.5, 2.0, 3.0)  # 0.002 / |rd| = 0.002, 0.00133, 0.001 (on the threshold: exempt by name), 0.00067


def _thin_rays(rng, n):
    o = np.stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), np.zeros(n)], -1)
    return o, np.float64([[0.0, 0.0, 1.0]]) * np.float64(THIN_LENGTHS)[np.arange(n) % 4][:, None]


_CENTRE = (0.0, 0.0, 3.0)


def _ball(radius, scale=(1.0, 1.0, 1.0)):
    return glam.mul(glam.mul(glam.from_translation(_CENTRE), glam.from_scale(scale)), glam.from_scale((radius,) * 3))


def _shells():
    """Concentric None spheres of radius 1, 0.6 and 0.3 around (0, 0, 3) with media 1, 2, 3 nested; an emitter at z = 6 faces the origin."""
    media = [None, _GREY1 + (0.0,), _CHROMA1 + (0.0,), _CHROMA2 + (0.0,)]
    return Description(media, [Ball(_ball(1.0), interior=1, exterior=0), Ball(_ball(0.6), interior=2, exterior=1), Ball(_ball(0.3), interior=3, exterior=2),
                               Rect(6, _BIG, _BIG, -1, material="matte", emit=_L)])


def _towards(rng, n, radius, scale=(1.0, 1.0, 1.0)):
    """From a sphere of radius 2.5 around the centre towards points of the solid of that radius (scaled)."""
    o = np.float64(_CENTRE) + 2.5 * br._sphere(rng, n)
    aim = np.float64(_CENTRE) + br._sphere(rng, n) * (radius * rng.uniform(0, 1, (n, 1)) ** (1 / 3)) * np.float64(scale)
    return o, br._unit(aim - o) * rng.choice([0.5, 1.0, 2.0], n)[:, None]


def _ellipsoid():
    """One None sphere under scale(1, 0.5, 2) around medium 1."""
    return Description([None, _CHROMA1 + (0.0,)], [Ball(_ball(1.0, (1.0, 0.5, 2.0)), interior=1, exterior=0), Rect(6, _BIG, _BIG, -1, material="matte", emit=_L)])


WALKS = {  # scene -> (the description, {start medium: the rays})
    "slabs": (_slabs, {m: _slabs_rays for m in range(5)}),
    "thin": (_thin, {0: _thin_rays}),
    "shells": (_shells, {0: lambda rng, n: _towards(rng, n, 1.0),
                         1: lambda rng, n: (np.float64(_CENTRE) + 0.8 * br._sphere(rng, n), br._sphere(rng, n) * rng.choice([0.5, 1.0, 2.0], n)[:, None]),
                         3: lambda rng, n: (np.tile(np.float64(_CENTRE), (n, 1)), br._sphere(rng, n) * rng.choice([0.5, 1.0, 2.0], n)[:, None])}),
    "ellipsoid": (_ellipsoid, {0: lambda rng, n: _towards(rng, n, 1.0, (1.0, 0.5, 2.0)),
                               1: lambda rng, n: (np.tile(np.float64(_CENTRE), (n, 1)), br._sphere(rng, n) * rng.choice([0.5, 1.0, 2.0], n)[:, None])}),
}
WALK_CASES = tuple((scene, start) for scene, (_, starts) in WALKS.items() for start in starts)
# Rows taken out of the cap's count, by name: (scene, start medium) -> (the rows, the reason)
WALK_EXEMPT = {("thin", 0): (lambda n: np.arange(n) % 4 == 2, "|rd| = 2 puts the pair 0.002 apart at t = 0.001, on the restart's tmin, by construction")}


@functools.lru_cache(None)
def walk_description(scene):
    return WALKS[scene][0]()


@functools.lru_cache(None)
def walk_rays(scene, start):
    rng = np.random.default_rng(9000 + 10 * list(WALKS).index(scene) + start)
    o, d = WALKS[scene][1][start](rng, N_WALK)
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)


@functools.lru_cache(None)
def walk_reference(scene, start, emit):
    o, d = walk_rays(scene, start)
    return walk(walk_description(scene), emit, start, o, d)


@functools.lru_cache(None)
def walk_scene(scene) -> Scene:
    """The description as a volpath Scene: rectangles as two-triangle meshes with their vertex normals, spheres as sphere instances."""
    D = walk_description(scene)
    s = Scene.new()
    s.integrator = abi.INTEGRATOR_VOLPATH
    s.set_camera(glam.look_at_lh((0.0, 0.0, -4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), 40.0, 16, 16)
    for m in D.media[1:]:
        s.add_medium_homogeneous(*m)
    matte = s.add_matte((0.5, 0.5, 0.5))
    for f in D.surfaces:
        material = 0 if f.material == "none" else matte
        light = s.add_area_light_diffuse(f.emit) if f.emit is not None else 0
        if isinstance(f, Rect):
            corners = [(f.x[0], f.y[0], f.z), (f.x[1], f.y[0], f.z), (f.x[1], f.y[1], f.z), (f.x[0], f.y[1], f.z)]
            mesh = TriangleMesh.from_arrays(corners, [0, 1, 2, 0, 2, 3], normals=[(0.0, 0.0, f.nz)] * 4)
            s.add_triangle_mesh(mesh, material, area_light=light, interior=f.interior, exterior=f.exterior)
        else:
            inst = s.add_sphere(1.0, material, area_light=light, interior=f.interior, exterior=f.exterior)
            s.instances[inst].matrix[:] = glam.affine_from_mat4(f.m.astype(np.float32))
    return s


def walk_check(rows, scene, start, emit):
    """rows (n, 4) in the layout of rene_transmittance: (worst error / allowance over the rays not set aside, the failing rays, the rays whose
    query count differs).  A ray set aside is held by class: finite, and within [0, the largest radiance]."""
    ref = walk_reference(scene, start, emit)
    rows = np.asarray(rows, np.float32)
    got = rows[:, 0:3].astype(np.float64)
    ratio = _ratio(got, ref.tr, ref.allow)
    top = max(_L) if emit else 1.0
    sane = np.isfinite(got).all(-1) & (got >= 0).all(-1) & (got <= top * (1 + 1e-5)).all(-1)
    bad = np.where(ref.aside, ~sane, ~(sane & (ratio <= 1.0)))
    count = ~ref.aside & (rows[:, 3].astype(np.int64) != ref.queries)
    keep = ~ref.aside
    return (float(ratio[keep].max()) if keep.any() else 0.0), bad, count


def walk_aside_share(scene, start, emit):
    ref = walk_reference(scene, start, emit)
    mask = ref.aside.copy()
    if (scene, start) in WALK_EXEMPT:
        mask &= ~WALK_EXEMPT[scene, start][0](len(mask))
    return float(mask.mean()), np.nonzero(mask)[0]
