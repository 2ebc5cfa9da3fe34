"""Restatement of the noise estimate (rene_estimate_noise, include/rene_hip.h) in plain numpy: the specification's three steps transcribed as
they are written, float64 by default.  A helper for tests (like atrous_reference.py): it does not import the library, and knows nothing of how
the device cuts the work.

    chain_sums [8][H][W][3]  the eight frame chains' radiance sums C_c         n_c [8]  frames each chain has received
"""
import numpy as np

CHAINS = 8
TILE = 32
LUM = (0.2126, 0.7152, 0.0722)
DEFAULT_FLOOR = 0.01

# 16 -> 64 frames must halve the figures.  The bands (noise, rel_rmse) are 1.5 x the widest deviation from 2 that the CPU oracle gave over
# eight master seeds (tests/test_noise_host.py reproduces the measurement and asserts it):
#   cornell_fog(64, 64)     noise 1.869 .. 2.167 (deviation 0.167 -> 0.25),  rel_rmse 1.919 .. 2.077 (0.081 -> 0.12)
#   cornell_box(100, 70)    noise 1.526 .. 2.243 (deviation 0.474 -> 0.71),  rel_rmse 1.918 .. 2.165 (0.165 -> 0.25)
# (Cornell's tile figure scatters more: its noise is concentrated in the few tiles around the light.)  The per-pixel ratio the header declines
# to offer gave 1.08 .. 1.21 on the fog scene and 0.91 .. 1.73 on Cornell for the same renders.
LAW_BANDS = {"fog": (0.25, 0.12), "cornell": (0.71, 0.25)}


def lum(v, f):
    return v[..., 0] * f(LUM[0]) + v[..., 1] * f(LUM[1]) + v[..., 2] * f(LUM[2])


def pixel_stats(chain_sums, n_c, dtype=np.float64):
    """Step 1: (l [H][W], var [H][W]) -- the luminance of the pixel's mean and the variance of that mean from the chains, in `dtype`."""
    f = dtype
    c = np.asarray(chain_sums).astype(f)
    n_c = np.asarray(n_c).astype(f)
    assert c.shape[0] == CHAINS and n_c.shape == (CHAINS,)
    n = f(n_c.sum())
    k = int((n_c > 0).sum())
    assert k >= 2
    s0 = c[0].copy()
    for g in range(1, CHAINS):  # ((C_0 + C_1) + ...) + C_7
        s0 = s0 + c[g]
    l = lum(s0 / n, f)
    var = np.zeros_like(l)
    for g in range(CHAINS):
        if n_c[g] > 0:
            lc = lum(c[g] / n_c[g], f)
            var = var + (n_c[g] / n) * (lc - l) ** 2
    return l, var / f(k - 1)


def tile_records(l, var):
    """Step 2's sums on the full grid: (A [ty][tx], B [ty][tx], n [ty][tx]) in the dtype of l and var."""
    h, w = l.shape
    ty, tx = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
    a, b, n = np.zeros((ty, tx), var.dtype), np.zeros((ty, tx), l.dtype), np.zeros((ty, tx), np.int64)
    for j in range(ty):
        for i in range(tx):
            sl = (slice(j * TILE, min(h, (j + 1) * TILE)), slice(i * TILE, min(w, (i + 1) * TILE)))
            a[j, i], b[j, i], n[j, i] = var[sl].sum(), l[sl].sum(), var[sl].size
    return a, b, n


def figures(a, b, n, floor=DEFAULT_FLOOR, owned=None):
    """Steps 2 and 3 from tile records (fp64): a dict with the fields of rene_noise_estimate and `tile_noise` [ty][tx].  `owned`: a boolean
    [ty][tx] mask of the tiles that count (a tile shard's), default all."""
    a, b, nn = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(n, np.float64)
    own = (nn > 0) if owned is None else (np.asarray(owned, bool) & (nn > 0))
    q = np.zeros_like(a)
    q[own] = (a[own] / nn[own]) / (b[own] / nn[own] + floor) ** 2
    tn = np.sqrt(q)
    n_px = nn[own].sum()
    worst = int(np.argmax(np.where(own, tn, -1.0)))  # the lowest index among equals
    return dict(n_tiles=int(own.sum()), n_pixels=int(n_px), sum_var=float(a[own].sum()), sum_lum=float(b[own].sum()),
                sum_weighted_q=float((nn[own] * q[own]).sum()), noise=float(np.sqrt((nn[own] * q[own]).sum() / n_px)),
                rel_rmse=float(np.sqrt(a[own].sum() / n_px) / (b[own].sum() / n_px + floor)),
                worst_tile_noise=float(tn.reshape(-1)[worst]), worst_tile=worst, tile_noise=tn)


def estimate(chain_sums, n_c, floor=DEFAULT_FLOOR, dtype=np.float64):
    """All three steps; per-pixel arithmetic and tile sums in `dtype`, the image-level sums in fp64 as the library's host side takes them."""
    l, var = pixel_stats(chain_sums, n_c, dtype)
    a, b, n = tile_records(l, var)
    out = figures(a, b, n, floor)
    out.update(A=a, B=b, n=n, l=l, var=var)
    return out


def per_pixel_ratio(l, var, floor=DEFAULT_FLOOR):
    """The metric the header declines to offer: mean over pixels of sd_p / (l_p + floor)."""
    return float(np.mean(np.sqrt(var) / (l + floor)))


def chains_of(renderer, spp, first=0, **render_kw):
    """The chains a job of frames first .. first + spp - 1 leaves, rebuilt frame by frame from anything with reset / render / download
    (frame f belongs to chain f % 8; each chain summed in frame order, fp32): (chain_sums, n_c)."""
    h, w = renderer.yres, renderer.xres
    chains = np.zeros((CHAINS, h, w, 3), np.float32)
    n_c = np.zeros(CHAINS)
    for fr in range(first, first + spp):
        renderer.reset()
        renderer.render(fr, 1, **render_kw)
        chains[fr % CHAINS] += renderer.download(0)
        n_c[fr % CHAINS] += 1
    return chains, n_c
