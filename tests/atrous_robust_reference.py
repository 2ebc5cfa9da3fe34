"""Restatement of the `atrous` denoiser's trimmed prepare (rene_denoise_robust, rene_denoise_tiles_robust, include/rene_hip.h) in plain numpy: the
contract transcribed as it is written, float64 by default.  Built on the other restatements -- steps R1 - R3 are robust_reference's, the filter's
taps and masks are atrous_tiles_reference's -- and, like them, a helper for tests that does not import the library and knows nothing of tiles:
the counts come per pixel, and a pixel is valid if its own counts fill two chains or more.

    chain_sums [8][H][W][3]  the eight frame chains' radiance sums C_c     n_c [8] or [8][H][W]  frames each chain has received
    s1, s2     [H][W][3]     the normal and albedo layers' sums

`decisions = (j, kept)`: the discrete half of the contract handed in, so that a float64 run can take the decisions of a float32 run (which are
the device's, bit for bit) and be compared with the device on the continuous half alone.
"""
import numpy as np

import atrous_reference as ar
import atrous_tiles_reference as at
import robust_reference as rr

CHAINS, DEFAULTS, lum = ar.CHAINS, ar.DEFAULTS, ar.lum
DEFAULT_MAX_TRIM = 3
DEFAULT_GAIN = 0.35


def per_pixel_counts(n_c, hw):
    n = np.asarray(n_c)
    return np.broadcast_to(n[:, None, None], (CHAINS,) + tuple(hw)).copy() if n.ndim == 1 else n


def trim(chain_sums, n_c, max_trim=DEFAULT_MAX_TRIM, gain=DEFAULT_GAIN, dtype=np.float64):
    """Steps R1 - R4 and the cap: (j [H][W] int, kept [8][H][W] bool).  Pixels with fewer than two non-empty chains: j = 0, everything kept."""
    f = dtype
    c = np.asarray(chain_sums).astype(f)
    hw = c.shape[1:3]
    n = per_pixel_counts(n_c, hw).astype(np.int64)
    assert c.shape[0] == CHAINS and n.shape == (CHAINS,) + hw and 0 <= max_trim <= 3
    j = np.zeros(hw, np.int64)
    kept = np.ones((CHAINS,) + hw, bool)
    for counts in np.unique(n.reshape(CHAINS, -1), axis=1).T:  # every distinct set of counts with the pixels that have it
        full = [g for g in range(CHAINS) if counts[g] > 0]
        k = len(full)
        if k < 2:
            continue
        m = (n == counts[:, None, None]).all(0)
        with np.errstate(all="ignore"):
            l = np.stack([rr.lum(c[g][m] / f(counts[g]), f) for g in full])  # R1: not demodulated
            rank, G = rr.gini(l, f)                                          # R2, R3
            t = (f(np.float32(gain)) * G) * (f(k) * f(0.5))                  # R4 (the library holds the gain as fp32)
            j0 = np.minimum(np.fmin(np.fmax(t, f(0)), f(3)).astype(np.int64), min(max_trim, (k - 1) // 2))
        jm = np.minimum(j0, (k - 2) // 2)  # at least two non-empty chains are kept
        j[m] = jm
        for i, g in enumerate(full):
            kept[g][m] = (rank[i] >= jm) & (rank[i] < k - jm)
    return j, kept


def denoise_robust(chain_sums, n_c, s1, s2, max_trim=DEFAULT_MAX_TRIM, gain=DEFAULT_GAIN, decisions=None, dtype=np.float64, **params):
    """A dict: `radiance` [H][W][3] (sums, the unit of rene_download), `mean` [H][W][3], `var` (the unfiltered plane), `valid`, `j`, `kept`.
    Invalid pixels as in atrous_tiles_reference.denoise_tiles: the unfiltered sums, the unfiltered mean (0 without frames), variance 0, j 0."""
    p = dict(DEFAULTS)
    p.update(params)
    f = dtype
    c = np.asarray(chain_sums).astype(f)
    hw = c.shape[1:3]
    s1 = np.asarray(s1).astype(f)
    s2 = np.asarray(s2).astype(f)
    n_c = per_pixel_counts(n_c, hw).astype(f)
    j, kept = trim(chain_sums, n_c, max_trim, gain, dtype) if decisions is None else decisions
    j, kept = np.asarray(j).astype(np.int64), np.asarray(kept).astype(bool)
    n = n_c.sum(0).astype(f)
    k = (n_c > 0).sum(0)
    valid = k >= 2
    j = np.where(valid, j, 0)
    one = f(1)
    s0 = c[0].copy()
    for g in range(1, CHAINS):  # ((C_0 + C_1) + ...) + C_7: what an invalid pixel hands out
        s0 = s0 + c[g]
    # 2'. the kept chains' sums in chain order, from C_0 or +0, and their frames
    acc = np.where(kept[0][..., None], c[0], f(0))
    n_kept = np.where(kept[0], n_c[0], f(0))
    for g in range(1, CHAINS):
        acc = np.where(kept[g][..., None], acc + c[g], acc)
        n_kept = np.where(kept[g], n_kept + n_c[g], n_kept)
    n_v = np.where(valid, n, one)[..., None]  # (invalid pixels are computed with harmless constants and selected away)
    nk_v = np.where(valid, n_kept, one)
    h = k - 2 * j
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # 1. guides: of the whole pixel
        alb = s2 / n_v
        nrm = s1 / n_v
        den = alb + f(p["albedo_floor"])
        d = (acc / nk_v[..., None]) / den
        l = lum(d, f)
        # 3'. variance of the mean from the kept chains
        var = np.zeros_like(l)
        for g in range(CHAINS):
            has = valid & kept[g] & (n_c[g] > 0)
            ng = np.where(has, n_c[g], one)
            lc = lum((c[g] / ng[..., None]) / den, f)
            var = np.where(has, var + (ng / nk_v) * (lc - l) ** 2, var)
        var = var / np.where(valid, h - 1, 1).astype(f)
        var0 = np.where(valid, var, f(0))
        # 4. the iterations, unchanged: a tap counts if it is inside the image and valid
        col = d
        for it in range(int(p["iterations"])):
            s = 1 << it
            g_, gw = np.zeros_like(var), np.zeros_like(var)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    w = f((2 - abs(dy)) * (2 - abs(dx)) / 16)
                    v, ok = at.masked_shift(var, valid, dy, dx)
                    g_ = g_ + w * v * ok
                    gw = gw + w * ok
            sd = f(p["sigma_luminance"]) * np.sqrt(np.maximum(g_ / gw, f(0)))
            lp = lum(col, f)
            a, av, wsum = np.zeros_like(col), np.zeros_like(var), np.zeros_like(var)
            for iy in range(5):
                for ix in range(5):
                    dy, dx = (iy - 2) * s, (ix - 2) * s
                    cq, ok = at.masked_shift(col, valid, dy, dx)
                    if not ok.any():
                        continue
                    nq, _ = at.masked_shift(nrm, valid, dy, dx)
                    aq, _ = at.masked_shift(alb, valid, dy, dx)
                    vq, _ = at.masked_shift(var, valid, dy, dx)
                    lq = lum(cq, f)
                    e = (((nrm - nq) ** 2).sum(-1) / f(p["sigma_normal2"]) + ((alb - aq) ** 2).sum(-1) / f(p["sigma_albedo2"])
                         + np.abs(lp - lq) / (sd + f(p["relative_floor"]) * (np.abs(lp) + np.abs(lq)) + f(1e-12)))
                    w = np.where(ok, f(ar.H5[ix] * ar.H5[iy]) * np.exp(-e), f(0))
                    a = a + w[..., None] * cq
                    av = av + w * w * vq
                    wsum = wsum + w
            col = a / wsum[..., None]
            var = av / wsum ** 2
        # 5. remodulate: the mean, and the sums over ALL the pixel's frames, whatever was trimmed
        mean = col * den
        radiance = col * den * n_v
        plain_mean = s0 / np.where(n > 0, n, one)[..., None]
    v3 = valid[..., None]
    return dict(radiance=np.where(v3, radiance, s0), mean=np.where(v3, mean, np.where((n > 0)[..., None], plain_mean, f(0))), var=var0,
                valid=valid, j=j, kept=kept)
