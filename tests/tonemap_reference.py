"""The tone-mapped output transform and the luminance histogram (include/rene_hip.h: rene_output_tonemapped, rene_luminance_histogram), restated
in numpy operation by operation: every intermediate is an fp32 array, so every `*`, `+`, `/` below rounds once to fp32, as the header says, and
nothing is fused.  The byte of the tone-mapped value is the count of sRGB thresholds at or below it (api.output_thresholds(), the table the
device looks its bytes up in).  The statistics are Python integers.  Tests compare bytes and counts with array_equal."""
import numpy as np

F = np.float32
CLAMP, REINHARD, ACES = 0, 1, 2
OPS = {"clamp": CLAMP, "reinhard": REINHARD, "aces": ACES}
FLT_MAX = np.finfo(np.float32).max
BINS = 256
E8_MIN, E8_MAX = -960, 960
M = [F(2.0 ** (k / 8.0)) for k in range(8)]  # what the header's eight literals must equal


def lum3(r, g, b):
    """chain_pass.h's luminance: (0.2126 r + 0.7152 g) + 0.0722 b."""
    return (F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b


def tonemap(means, op, scale, white):
    """[..., >= 3] fp32 means -> [..., 3] fp32 values whose sRGB bytes are the image."""
    v = np.asarray(means, np.float32)[..., :3]
    with np.errstate(all="ignore"):
        e = v * F(scale)
        if op == CLAMP:
            return e
        if op == REINHARD:
            w2 = F(white) * F(white)
            l = np.fmin(np.fmax(lum3(e[..., 0], e[..., 1], e[..., 2]), F(0)), FLT_MAX)
            q = l / w2
            a = F(1) + q
            b = F(1) + l
            f = a / b
            return e * f[..., None]
        if op == ACES:
            x = np.fmin(np.fmax(e, F(0)), F(16777216.0))
            n = x * (F(2.51) * x + F(0.03))
            d = x * (F(2.43) * x + F(0.59)) + F(0.14)
            return n / d
    raise ValueError(op)


def srgb_bytes(c, thresholds):
    """The byte of every value: the number of thresholds <= it (a NaN counts none)."""
    c = np.asarray(c, np.float32)
    with np.errstate(invalid="ignore"):
        return np.searchsorted(thresholds, np.where(np.isnan(c), F(-1), c), "right").astype(np.uint8)


def tonemap_rgb8(means, op, scale, white, thresholds):
    return srgb_bytes(tonemap(means, op, scale, white), thresholds)


def luminance_bins(l):
    """The bin of every luminance (an int array; -1: counted dark)."""
    l = np.ascontiguousarray(l, np.float32)
    bits = l.view(np.uint32).astype(np.int64)
    with np.errstate(invalid="ignore"):
        lit = l > 0
    return np.where(lit, np.clip((bits >> 20) - 856, 0, BINS - 1), -1)


def histogram(means):
    """(counts[256], n_dark) of [..., >= 3] means: the luminance of the un-exposed mean."""
    v = np.asarray(means, np.float32)
    with np.errstate(all="ignore"):
        b = luminance_bins(lum3(v[..., 0], v[..., 1], v[..., 2])).reshape(-1)
    return np.bincount(b[b >= 0], minlength=BINS).astype(np.uint32), int((b < 0).sum())


def mean_bin_x256(counts):
    n_lit = sum(int(c) for c in counts)
    return sum(int(c) * (2 * b + 1) for b, c in enumerate(counts)) * 128 // n_lit if n_lit else 0


def percentile_bin(counts, per_mille):
    n_lit = sum(int(c) for c in counts)
    if n_lit == 0:
        return -1
    need, run = (n_lit * per_mille + 999) // 1000, 0
    for b, c in enumerate(counts):
        run += int(c)
        if run >= need:
            return b
    return BINS - 1


def auto_exposure_e8(counts, key_e8=-20):
    if not sum(int(c) for c in counts):
        return 0
    return max(E8_MIN, min(E8_MAX, key_e8 + 160 - ((mean_bin_x256(counts) + 128) >> 8)))


def exposure_scale(e8):
    e8 = max(E8_MIN, min(E8_MAX, int(e8)))
    return F(np.ldexp(M[e8 & 7], e8 >> 3))  # (Python's & and >> on a negative int are the floor forms the header means)


def bin_edges():
    """Every edge 2^k (1 + j / 8) of the histogram's bins, 2^-20 .. 2^12 inclusive: exact fp32 values."""
    return np.array([np.ldexp(1.0 + j / 8.0, k) for k in range(-20, 12) for j in range(8)] + [4096.0], np.float32)


# ---- the value sets the CPU and the GPU tests share ---------------------------------------------------------------------------------------------
SPECIALS = np.array([0.0, -0.0, -1.0, -1e-30, -1e30, 1e-45, -1e-45, 1e-39, 1.1754942e-38, np.nan, -np.nan, np.inf, -np.inf, 1e30, 0.0031308,
                     np.nextafter(F(0.0031308), F(1)), 1.0, np.nextafter(F(1), F(0)), 1.5, 3.4e38, -3.4e38, 4.0, 16.0, 16777216.0, 2e7], np.float32)
SCALES = [F(1), F(2 ** (3 / 8)), F(2 ** -3)]


def around(t, ulps=2):
    out = [t]
    lo = hi = t
    for _ in range(ulps):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        out += [lo, hi]
    return np.concatenate(out).astype(np.float32)


def value_set(T):
    """The values every tone-map test runs on, here and on the GPU: the 255 thresholds and their neighbours, the specials, and every 4096th bit
    pattern from +0 up to 2^13 -- as [n][3] pixels: grey, each value alone in a channel beside 0.25 and 2, and against the specials."""
    strided = np.arange(0, 0x46000000, 4096, dtype=np.uint32).view(np.float32)
    assert strided[-1] < 8192.0 and strided.size > 280000
    v = np.concatenate([around(T), SPECIALS, strided])
    grey = np.stack([v, v, v], -1)
    mixed = np.stack([v, np.full_like(v, 0.25), np.full_like(v, 2.0)], -1)
    rolled = np.stack([np.roll(v, 1), v, np.roll(v, -1)], -1)[:8192]
    sp = np.stack(np.meshgrid(SPECIALS, SPECIALS, SPECIALS, indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([grey, mixed, rolled, sp]), dtype=np.float32)


def edge_pixels():
    """Pixels whose luminance is exactly an edge 2^k (1 + j / 8) of the histogram's bins, the float below it or the float above it, for every k
    from -20 to 12.  lum3 of (r, g, b) x 2^k is lum3(r, g, b) x 2^k exactly (no product here is a denormal), so the 24 pixels of one octave are
    found once -- r and b at random, g solved for in double and rounded, which lands within an ulp or two of the target: one of 4096 tries hits
    it -- and scaled."""
    rng = np.random.default_rng(11)
    octave = []
    for j in range(8):
        e = F(1 + j / 8)
        for t in (np.nextafter(e, F(0)), e, np.nextafter(e, F(2))):
            r, b = rng.random(4096, np.float32), rng.random(4096, np.float32)
            g = ((np.float64(t) - 0.2126 * r - 0.0722 * b) / 0.7152).astype(np.float32)
            px = np.stack([r, g, b], -1)
            hit = np.flatnonzero(lum3(r, g, b) == t)
            assert hit.size, (j, float(t))
            octave.append(px[hit[0]])
    octave = np.array(octave, np.float32)
    return np.concatenate([np.ldexp(octave, k).astype(np.float32) for k in range(-20, 13)])
