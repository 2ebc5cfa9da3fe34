"""Restatement of the `atrous` denoiser tile by tile (rene_denoise_tiles, include/rene_hip.h) in plain numpy: the contract transcribed as it is
written, float64 by default.  A helper for tests (like atrous_reference.py, whose steps it repeats with the counts per pixel): it does not import
the library, and knows nothing of tiles -- a pixel is valid if its own counts fill two chains or more.

    chain_sums [8][H][W][3]  the eight frame chains' radiance sums C_c     n_c [8][H][W]  frames each chain has received, per pixel
    s1, s2     [H][W][3]     the normal and albedo layers' sums
"""
import numpy as np

import atrous_reference as ar

CHAINS, H5, DEFAULTS, lum, shift = ar.CHAINS, ar.H5, ar.DEFAULTS, ar.lum, ar.shift
TILE = 32


def chain_counts(first, n):
    """n_c [8] of the frames first .. first + n - 1 (frame f belongs to chain f % 8)."""
    out = np.zeros(CHAINS)
    for f in range(first, first + n):
        out[f % CHAINS] += 1
    return out


def per_pixel(tile_values, yres, xres):
    """[...][ty][tx] -> [...][H][W]: every tile's value on its 32 x 32 pixels, clipped to the image."""
    v = np.asarray(tile_values)
    return np.repeat(np.repeat(v, TILE, axis=-2), TILE, axis=-1)[..., :yres, :xres]


def masked_shift(a, ok_in, dy, dx):
    """shift() of `a` with the taps that are outside the image OR not `ok_in` at their source set to 0 by selection (whatever they hold)."""
    b, inside = shift(a, dy, dx)
    v, _ = shift(ok_in, dy, dx)
    ok = inside & v
    return np.where(ok[(...,) + (None,) * (b.ndim - 2)], b, 0), ok


def denoise_tiles(chain_sums, n_c, s1, s2, dtype=np.float64, **params):
    """(radiance sums [H][W][3] in the unit of rene_download, the mean [H][W][3], the unfiltered variance plane [H][W], valid [H][W]), in `dtype`.
    Invalid pixels: the unfiltered sums, the unfiltered sums over their frame count (0 without frames), variance 0."""
    p = dict(DEFAULTS)
    p.update(params)
    f = dtype
    c = np.asarray(chain_sums).astype(f)
    s1 = np.asarray(s1).astype(f)
    s2 = np.asarray(s2).astype(f)
    n_c = np.asarray(n_c).astype(f)
    assert c.shape[0] == CHAINS and n_c.shape == c.shape[:3]
    n = n_c.sum(0).astype(f)
    k = (n_c > 0).sum(0)
    valid = k >= 2
    s0 = c[0].copy()
    for g in range(1, CHAINS):  # ((C_0 + C_1) + ...) + C_7
        s0 = s0 + c[g]
    one = f(1)
    n_v = np.where(valid, n, one)[..., None]  # (invalid pixels are computed with harmless constants and selected away)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # 1. guides
        alb = s2 / n_v
        nrm = s1 / n_v
        den = alb + f(p["albedo_floor"])
        # 2. demodulated colour
        d = (s0 / n_v) / den
        l = lum(d, f)
        # 3. variance of the mean from the chains
        var = np.zeros_like(l)
        for g in range(CHAINS):
            has = valid & (n_c[g] > 0)
            ng = np.where(has, n_c[g], one)
            lc = lum((c[g] / ng[..., None]) / den, f)
            var = np.where(has, var + (ng / n_v[..., 0]) * (lc - l) ** 2, var)
        var = var / np.where(valid, k - 1, 1).astype(f)
        var0 = np.where(valid, var, f(0))
        # 4. the iterations: a tap counts if it is inside the image and valid
        col = d
        for it in range(int(p["iterations"])):
            s = 1 << it
            g_, gw = np.zeros_like(var), np.zeros_like(var)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    w = f((2 - abs(dy)) * (2 - abs(dx)) / 16)
                    v, ok = masked_shift(var, valid, dy, dx)
                    g_ = g_ + w * v * ok
                    gw = gw + w * ok
            sd = f(p["sigma_luminance"]) * np.sqrt(np.maximum(g_ / gw, f(0)))
            lp = lum(col, f)
            acc, accv, wsum = np.zeros_like(col), np.zeros_like(var), np.zeros_like(var)
            for iy in range(5):
                for ix in range(5):
                    dy, dx = (iy - 2) * s, (ix - 2) * s
                    cq, ok = masked_shift(col, valid, dy, dx)
                    if not ok.any():
                        continue
                    nq, _ = masked_shift(nrm, valid, dy, dx)
                    aq, _ = masked_shift(alb, valid, dy, dx)
                    vq, _ = masked_shift(var, valid, dy, dx)
                    lq = lum(cq, f)
                    e = (((nrm - nq) ** 2).sum(-1) / f(p["sigma_normal2"]) + ((alb - aq) ** 2).sum(-1) / f(p["sigma_albedo2"])
                         + np.abs(lp - lq) / (sd + f(p["relative_floor"]) * (np.abs(lp) + np.abs(lq)) + f(1e-12)))
                    w = np.where(ok, f(H5[ix] * H5[iy]) * np.exp(-e), f(0))
                    acc = acc + w[..., None] * cq
                    accv = accv + w * w * vq
                    wsum = wsum + w
            col = acc / wsum[..., None]
            var = accv / wsum ** 2
        # 5. remodulate: the mean, and the sums over the pixel's own frames
        mean = col * den
        radiance = col * den * n_v
        plain_mean = s0 / np.where(n > 0, n, one)[..., None]
    v3 = valid[..., None]
    return np.where(v3, radiance, s0), np.where(v3, mean, np.where((n > 0)[..., None], plain_mean, f(0))), var0, valid


def compose(parts, tile_class, yres, xres):
    """One film from uniform ones: parts {class: (chain_sums [8][H][W][3], n_c [8], s1, s2)}, tile_class [ty][tx] -> (chain_sums, n_c [8][H][W],
    s1, s2), every tile taken from the film of its class."""
    classes = sorted(parts)
    index = per_pixel(np.vectorize(classes.index)(tile_class), yres, xres)
    chains = np.zeros((CHAINS, yres, xres, 3), np.float32)
    n_c = np.zeros((CHAINS, yres, xres))
    s1, s2 = np.zeros((yres, xres, 3), np.float32), np.zeros((yres, xres, 3), np.float32)
    for i, cl in enumerate(classes):
        pc, pn, p1, p2 = parts[cl]
        m = index == i
        chains[:, m] = np.asarray(pc)[:, m]
        n_c[:, m] = np.asarray(pn)[:, None]
        s1[m], s2[m] = np.asarray(p1)[m], np.asarray(p2)[m]
    return chains, n_c, s1, s2


# ---- the schedule the tests share: five classes of tiles, two of them invalid -------------------------------------------------------------------
# class A is switched off before the first render (no frames: invalid), B after a launch of ONE frame (one chain: invalid), C after 10 more, D after
# 8 more, E renders the last 16 too: chains of unequal length (11 = 8 + 3, 19 = 16 + 3, 35 = 32 + 3)
CLASS_FRAMES = {"A": 0, "B": 1, "C": 11, "D": 19, "E": 35}
LAUNCHES = (1, 10, 8, 16)


def tile_classes(xres, yres):
    """[ty][tx] of 'A' .. 'E': class (x + 3 y) mod 5 -- all five present from a 3 x 2 grid on."""
    ty, tx = (yres + TILE - 1) // TILE, (xres + TILE - 1) // TILE
    return np.array([["ABCDE"[(x + 3 * y) % 5] for x in range(tx)] for y in range(ty)])


def class_frames(classes):
    return np.vectorize(CLASS_FRAMES.get)(classes).astype(np.uint32)


def run_schedule(r, classes, cuts=None):
    """The masked job on anything with set_active_tiles / render: A off, 1 frame, B off, 10 frames, C off, 8 frames, D off, 16 frames.  cuts: a
    launch's frames in that many render calls."""
    mask = classes != "A"
    r.set_active_tiles(mask)
    done = 0
    for n, drop in zip(LAUNCHES, "BCD "):
        for part in np.array_split(np.arange(n), min(n, cuts or 1)):
            r.render(done, len(part))
            done += len(part)
        if drop != " ":
            mask = mask & (classes != drop)
            r.set_active_tiles(mask)


def chains_by_count(renderer, counts, **render_kw):
    """{N: (chain_sums, n_c [8], s1, s2)} of the jobs of frames 0 .. N - 1, N in counts, rebuilt frame by frame from anything with reset / render /
    download, like atrous_reference.chains_of (each chain summed in frame order, fp32) -- one pass over the frames for all the counts."""
    h, w = renderer.yres, renderer.xres
    chains = np.zeros((CHAINS, h, w, 3), np.float32)
    s1 = np.zeros((h, w, 3), np.float32)
    s2 = np.zeros((h, w, 3), np.float32)
    out = {0: (chains.copy(), chain_counts(0, 0), s1.copy(), s2.copy())} if 0 in counts else {}
    for fr in range(max(counts)):
        renderer.reset()
        renderer.render(fr, 1, **render_kw)
        chains[fr % CHAINS] += renderer.download(0)
        s1 += renderer.download(1)
        s2 += renderer.download(2)
        if fr + 1 in counts:
            out[fr + 1] = (chains.copy(), chain_counts(0, fr + 1), s1.copy(), s2.copy())
    return out
