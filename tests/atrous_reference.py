"""Restatement of the `atrous` denoiser (rene_denoise, include/rene_hip.h) in plain numpy: the specification's five steps transcribed as they
are written, float64 by default.  A helper for tests (like t2_regions.py): it does not import the library, and knows nothing of how the device
cuts the work.

    chain_sums [8][H][W][3]  the eight frame chains' radiance sums C_c         n_c [8]  frames each chain has received
    s1, s2     [H][W][3]     the normal and albedo layers' sums
"""
import numpy as np

CHAINS = 8
LUM = (0.2126, 0.7152, 0.0722)
H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_normal2=1 / 64, sigma_albedo2=1 / 16, albedo_floor=0.05, relative_floor=1e-3)


def shift(a, dy, dx):
    """(b, ok): b[y, x] = a[y + dy, x + dx] where that lies inside the image (ok), 0 elsewhere."""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    ok = np.zeros((h, w), bool)
    y0, y1 = max(0, dy), min(h, h + dy)
    x0, x1 = max(0, dx), min(w, w + dx)
    if y0 < y1 and x0 < x1:
        out[y0 - dy:y1 - dy, x0 - dx:x1 - dx] = a[y0:y1, x0:x1]
        ok[y0 - dy:y1 - dy, x0 - dx:x1 - dx] = True
    return out, ok


def lum(v, f):
    return v[..., 0] * f(LUM[0]) + v[..., 1] * f(LUM[1]) + v[..., 2] * f(LUM[2])


def denoise(chain_sums, n_c, s1, s2, dtype=np.float64, **params):
    """(radiance sums [H][W][3] in the unit of rene_download, unfiltered variance plane [H][W]), computed in `dtype`."""
    p = dict(DEFAULTS)
    p.update(params)
    f = dtype
    c = np.asarray(chain_sums).astype(f)
    s1 = np.asarray(s1).astype(f)
    s2 = np.asarray(s2).astype(f)
    n_c = np.asarray(n_c).astype(f)
    assert c.shape[0] == CHAINS and n_c.shape == (CHAINS,)
    n = f(n_c.sum())
    k = int((n_c > 0).sum())
    assert k >= 2
    s0 = c[0].copy()
    for g in range(1, CHAINS):  # ((C_0 + C_1) + ...) + C_7
        s0 = s0 + c[g]
    # 1. guides
    alb = s2 / n
    nrm = s1 / n
    den = alb + f(p["albedo_floor"])
    # 2. demodulated colour
    d = (s0 / n) / den
    l = lum(d, f)
    # 3. variance of the mean from the chains
    var = np.zeros_like(l)
    for g in range(CHAINS):
        if n_c[g] > 0:
            lc = lum((c[g] / n_c[g]) / den, f)
            var = var + (n_c[g] / n) * (lc - l) ** 2
    var = var / f(k - 1)
    var0 = var.copy()
    # 4. the iterations
    col = d
    for it in range(int(p["iterations"])):
        s = 1 << it
        g_, gw = np.zeros_like(var), np.zeros_like(var)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                w = f((2 - abs(dy)) * (2 - abs(dx)) / 16)
                v, ok = shift(var, dy, dx)
                g_ = g_ + w * v * ok
                gw = gw + w * ok
        sd = f(p["sigma_luminance"]) * np.sqrt(np.maximum(g_ / gw, f(0)))
        lp = lum(col, f)
        acc, accv, wsum = np.zeros_like(col), np.zeros_like(var), np.zeros_like(var)
        for iy in range(5):
            for ix in range(5):
                dy, dx = (iy - 2) * s, (ix - 2) * s
                cq, ok = shift(col, dy, dx)
                if not ok.any():
                    continue
                nq, _ = shift(nrm, dy, dx)
                aq, _ = shift(alb, dy, dx)
                vq, _ = shift(var, dy, dx)
                lq = lum(cq, f)
                e = (((nrm - nq) ** 2).sum(-1) / f(p["sigma_normal2"]) + ((alb - aq) ** 2).sum(-1) / f(p["sigma_albedo2"])
                     + np.abs(lp - lq) / (sd + f(p["relative_floor"]) * (np.abs(lp) + np.abs(lq)) + f(1e-12)))
                w = f(H5[ix] * H5[iy]) * np.exp(-e) * ok
                acc = acc + w[..., None] * cq
                accv = accv + w * w * vq
                wsum = wsum + w
        col = acc / wsum[..., None]
        var = accv / wsum ** 2
    # 5. remodulate, in sums
    return col * den * n, var0


def relmse(x, r):
    x, r = np.asarray(x, np.float64), np.asarray(r, np.float64)
    return float(np.mean((x - r) ** 2 / (r ** 2 + 1e-2)))


def chains_of(renderer, spp, first=0, **render_kw):
    """The chains a job of frames first .. first + spp - 1 leaves, rebuilt frame by frame from anything with reset / render / download
    (frame f belongs to chain f % 8; each chain summed in frame order, fp32): (chain_sums, n_c, s1, s2)."""
    h, w = renderer.yres, renderer.xres
    chains = np.zeros((CHAINS, h, w, 3), np.float32)
    n_c = np.zeros(CHAINS)
    s1 = np.zeros((h, w, 3), np.float32)
    s2 = np.zeros((h, w, 3), np.float32)
    for fr in range(first, first + spp):
        renderer.reset()
        renderer.render(fr, 1, **render_kw)
        chains[fr % CHAINS] += renderer.download(0)
        n_c[fr % CHAINS] += 1
        s1 += renderer.download(1)
        s2 += renderer.download(2)
    return chains, n_c, s1, s2
