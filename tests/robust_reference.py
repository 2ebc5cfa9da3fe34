"""Restatement of the firefly-robust resolve (rene_resolve_robust, include/rene_hip.h) in plain numpy: the specification's six steps transcribed
as they are written, float64 by default.  In np.float32 every operation is individually rounded and none is fused -- what the specification asks
of the device -- so the device's pixels can be held to it bit for bit.  A helper for tests (like noise_reference.py): it does not import the
library, and knows nothing of how the device cuts the work.

    chain_sums [8][H][W][3]  the eight frame chains' radiance sums C_c         n_c [8]  frames each chain has received
"""
import numpy as np

CHAINS = 8
TILE = 32
LUM = (0.2126, 0.7152, 0.0722)
DEFAULT_MAX_TRIM = 3
DEFAULT_GAIN = 1.0


def lum(v, f):
    return (f(LUM[0]) * v[..., 0] + f(LUM[1]) * v[..., 1]) + f(LUM[2]) * v[..., 2]


def gini(l, f):
    """Steps 2 and 3 for luminances l [k][...] of the k non-empty chains, in chain order: (ranks [k][...] int, G [...])."""
    k = l.shape[0]
    rank = np.zeros(l.shape, np.int64)
    for a in range(k):
        for b in range(k):
            if a != b:
                rank[a] += (l[b] < l[a]) | ((l[b] == l[a]) & (b < a))
    tot = np.zeros(l.shape[1:], f)
    num = np.zeros(l.shape[1:], f)
    for a in range(k):
        tot = tot + l[a]
        num = num + (2 * rank[a] + 1 - k).astype(f) * l[a]
    with np.errstate(all="ignore"):
        g = np.where(tot > 0, num / (f(k) * tot), f(0))
    return rank, g.astype(f)


def resolve(chain_sums, n_c, max_trim=DEFAULT_MAX_TRIM, gain=DEFAULT_GAIN, dtype=np.float64):
    """All six steps per pixel: a dict with `image` [H][W][3] (the robust mean), `j` [H][W] (int), `plain` [H][W][3] (S0 / N), `G` [H][W],
    `lum_plain` and `lum_robust` [H][W], everything floating in `dtype`."""
    f = dtype
    c = np.asarray(chain_sums).astype(f)
    n = np.asarray(n_c).astype(np.int64)
    assert c.shape[0] == CHAINS and n.shape == (CHAINS,) and 0 <= max_trim <= 3
    hw = c.shape[1:3]
    total = int(n.sum())
    if total == 0:
        z = np.zeros(hw + (3,), f)
        return dict(image=z, j=np.zeros(hw, np.int64), plain=z.copy(), G=np.zeros(hw, f), lum_plain=np.zeros(hw, f), lum_robust=np.zeros(hw, f))
    full = [g for g in range(CHAINS) if n[g] > 0]
    k = len(full)
    with np.errstate(all="ignore"):
        l = np.stack([lum(c[g] / f(n[g]), f) for g in full])  # step 1
        rank, G = gini(l, f)                                  # steps 2, 3
        t = (f(np.float32(gain)) * G) * (f(k) * f(0.5))       # step 4 (the library holds the gain as fp32)
        j = np.minimum(np.fmin(np.fmax(t, f(0)), f(3)).astype(np.int64), min(max_trim, (k - 1) // 2))  # (fmax / fmin: a NaN counts as 0)
        acc = np.zeros(hw + (3,), f)                          # step 5
        s0 = np.zeros(hw + (3,), f)
        n_kept = np.zeros(hw, np.int64)
        for g in range(CHAINS):
            s0 = s0 + c[g]
            if n[g] == 0:
                acc = acc + c[g]  # zeros: exact
                continue
            r = rank[full.index(g)]
            kept = (r >= j) & (r < k - j)
            acc = np.where(kept[..., None], acc + c[g], acc)
            n_kept += np.where(kept, n[g], 0)
        image = acc / n_kept.astype(f)[..., None]
        plain = s0 / f(total)
    return dict(image=image, j=j, plain=plain, G=G, lum_plain=lum(plain, f), lum_robust=lum(image, f))


def tile_records(lum_plain, lum_robust, j):
    """The tile records on the full grid: (sum_lum_plain, sum_lum_robust [ty][tx] in the inputs' dtype, n_pixels, n_trimmed [ty][tx] int)."""
    h, w = j.shape
    ty, tx = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
    a, b = np.zeros((ty, tx), lum_plain.dtype), np.zeros((ty, tx), lum_robust.dtype)
    n, nt = np.zeros((ty, tx), np.int64), np.zeros((ty, tx), np.int64)
    for y in range(ty):
        for x in range(tx):
            sl = (slice(y * TILE, min(h, (y + 1) * TILE)), slice(x * TILE, min(w, (x + 1) * TILE)))
            a[y, x], b[y, x], n[y, x], nt[y, x] = lum_plain[sl].sum(), lum_robust[sl].sum(), j[sl].size, int((j[sl] > 0).sum())
    return a, b, n, nt


def summary(a, b, n, nt, owned=None):
    """rene_robust_summary's additive fields and kept_energy from tile records (fp64, in tile order).  `owned`: a boolean [ty][tx] mask of the
    tiles that count (a tile shard's), default all."""
    own = (np.asarray(n) > 0) if owned is None else (np.asarray(owned, bool) & (np.asarray(n) > 0))
    sp = sr = 0.0
    for p, r in zip(np.asarray(a, np.float64)[own].reshape(-1), np.asarray(b, np.float64)[own].reshape(-1)):
        sp += float(p)
        sr += float(r)
    return dict(n_tiles=int(own.sum()), n_pixels=int(np.asarray(n)[own].sum()), n_trimmed=int(np.asarray(nt)[own].sum()), sum_lum_plain=sp,
                sum_lum_robust=sr, kept_energy=sr / sp if sp != 0.0 else 1.0)


def chain_counts(spp, first=0):
    """n_c of frames first .. first + spp - 1 (frame f belongs to chain f % 8)."""
    n = np.zeros(CHAINS, np.int64)
    for fr in range(first, first + spp):
        n[fr % CHAINS] += 1
    return n
