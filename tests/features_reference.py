"""Restatement of the denoiser hand-off's arithmetic (rene_export_features, include/rene_hip.h) in plain numpy: one statement per operation, as
the specification writes them.  In np.float32 every operation is individually rounded and none is fused -- what the specification asks of the
device -- so the device's tensor can be held to it bit for bit; in np.float64 it is the yardstick of the fp32 rounding.  A helper for tests
(like robust_reference.py): it does not import the library, and knows nothing of how the device cuts the work.

    chain_sums [8][H][W][3]  the eight frame chains' radiance sums C_c         n_c [8]  frames each chain has received
    s_normal, s_albedo [H][W][3]  the resolved sums of layers 1 and 2 (None: zeros)
"""
import numpy as np

CHAINS = 8
TILE = 32
LUM = (0.2126, 0.7152, 0.0722)
COLOR, ALBEDO, NORMAL, VARIANCE, HALF_A, HALF_B, FRAMES = (1 << b for b in range(7))
ALL = 127
DEFAULT = COLOR | ALBEDO | NORMAL
NAMES = {COLOR: "color", ALBEDO: "albedo", NORMAL: "normal", VARIANCE: "variance", HALF_A: "half_a", HALF_B: "half_b", FRAMES: "frames"}
WIDTH = {COLOR: 3, ALBEDO: 3, NORMAL: 3, VARIANCE: 1, HALF_A: 3, HALF_B: 3, FRAMES: 1}
F16_MAX = 65504.0
# The fp32-vs-fp64 spread of this restatement's VARIANCE tile sums on the CPU oracle's chains of SPREAD_CASES (scene of rene_amd.scenes, its
# arguments, frames), as max over tiles of |fp32 - fp64| / (|fp64| + the largest tile's value), the fp32 pixels summed in fp64 / in fp32:
#   3.0e-8 / 7.2e-9, 2.1e-8 / 3.7e-8, 1.7e-8 / 1.4e-8, 3.6e-8 / 4.5e-8
# tests/test_features_host.py reproduces the measurement and holds it to the largest; tests/test_gpu_features.py takes 16 x it as a one-sided bound.
VARIANCE_SPREAD = 4.5e-8
SPREAD_CASES = {"cornell-12": ("cornell_box", (100, 70), 12), "cornell-5": ("cornell_box", (100, 70), 5), "fog": ("cornell_fog", (64, 64), 12),
                "dragon": ("dragon_class", (96, 64, 20, 22), 12)}


def channels(mask):
    """rene_feature_channels: the channels a mask selects, 0 for an empty mask or unknown bits."""
    if mask == 0 or mask & ~ALL:
        return 0
    return sum(w for bit, w in WIDTH.items() if mask & bit)


def channel_slices(mask):
    """{bit: slice of the channel axis} for the features of the mask, in bit order."""
    out, at = {}, 0
    for bit in sorted(WIDTH):
        if mask & bit:
            out[bit] = slice(at, at + WIDTH[bit])
            at += WIDTH[bit]
    return out


def lum(v, f):
    return (f(LUM[0]) * v[..., 0] + f(LUM[1]) * v[..., 1]) + f(LUM[2]) * v[..., 2]


def features(chain_sums, n_c, s_normal=None, s_albedo=None, dtype=np.float32):
    """Every feature per pixel: {bit: [H][W][3] or [H][W]} in `dtype`."""
    f = dtype
    c = np.asarray(chain_sums).astype(f)
    n = np.asarray(n_c).astype(np.int64)
    assert c.shape[0] == CHAINS and n.shape == (CHAINS,)
    hw = c.shape[1:3]
    total = int(n.sum())
    z3, z1 = np.zeros(hw + (3,), f), np.zeros(hw, f)
    if total == 0:  # a tile without frames is all zeros
        return {COLOR: z3, ALBEDO: z3.copy(), NORMAL: z3.copy(), VARIANCE: z1, HALF_A: z3.copy(), HALF_B: z3.copy(), FRAMES: z1.copy()}
    nf = f(total)
    out = {}
    with np.errstate(all="ignore"):
        s0 = c[0] + c[1]
        for g in range(2, CHAINS):
            s0 = s0 + c[g]
        color = s0 / nf
        out[COLOR] = color
        out[ALBEDO] = (z3 if s_albedo is None else np.asarray(s_albedo).astype(f)) / nf
        out[NORMAL] = (z3 if s_normal is None else np.asarray(s_normal).astype(f)) / nf
        for bit, first in ((HALF_A, 0), (HALF_B, 1)):
            n_half = int(n[first] + n[first + 2] + n[first + 4] + n[first + 6])
            if n_half == 0:
                out[bit] = z3.copy()
                continue
            acc = c[first] + c[first + 2]
            acc = acc + c[first + 4]
            acc = acc + c[first + 6]
            out[bit] = acc / f(n_half)
        k = int((n > 0).sum())
        v = np.zeros(hw, f)
        if k >= 2:
            l = lum(color, f)
            for g in range(CHAINS):
                if n[g] == 0:
                    continue
                m = c[g] / f(n[g])
                t = lum(m, f) - l
                share = f(n[g]) / nf
                v = v + share * (t * t)
            v = v / f(k - 1)
        out[VARIANCE] = v
        out[FRAMES] = np.full(hw, nf, f)
    return out


def tensor(feats, mask, layout="hwc"):
    """The features of the mask in bit order as one [H][W][C] or [C][H][W] array."""
    planes = []
    for bit in sorted(WIDTH):
        if mask & bit:
            planes.append(feats[bit] if WIDTH[bit] == 3 else feats[bit][..., None])
    t = np.concatenate(planes, axis=-1)
    assert t.shape[-1] == channels(mask)
    return np.ascontiguousarray(t if layout == "hwc" else np.moveaxis(t, -1, 0))


def to_f16(x):
    """RENE_FEATURES_F16 of an fp32 result: clamped to the finite halves, rounded to nearest even, subnormals kept; a NaN stays one."""
    return np.clip(x, np.float32(-F16_MAX), np.float32(F16_MAX)).astype(np.float16)


def chain_counts(spp, first=0):
    """n_c of frames first .. first + spp - 1 (frame f belongs to chain f % 8)."""
    n = np.zeros(CHAINS, np.int64)
    for fr in range(first, first + spp):
        n[fr % CHAINS] += 1
    return n


def tile_sums(plane, dtype=np.float64):
    """[ty][tx] sums of a [H][W] plane over the 32 x 32 tiles, accumulated in `dtype` in row-major pixel order."""
    h, w = plane.shape
    ty, tx = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
    out = np.zeros((ty, tx), dtype)
    for y in range(ty):
        for x in range(tx):
            out[y, x] = plane[y * TILE:(y + 1) * TILE, x * TILE:(x + 1) * TILE].astype(dtype).sum(dtype=dtype)
    return out
