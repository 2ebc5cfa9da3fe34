"""What the tests of the passes over the eight frame chains share (rene_load_chains, include/rene_hip.h, puts such chains on the device): the
tile reduction of rene_amd/csrc/chain_pass.h restated in numpy, the slot <-> pixel map of a tile, a film of crafted chains whose pixels sit on
the edges the header makes promises about, and the fp32 values around every rounding boundary of fp16.  A helper for tests (like
robust_reference.py): it does not import the library.

    chains [8][3][H][W][3]  chain, layer (0 radiance, 1 normal, 2 albedo), rows top first, RGB -- the layout rene_load_chains takes
"""
import numpy as np

CHAINS = 8
TILE = 32
SLOTS = TILE * TILE
BLOCK = 256          # threads of a pass's workgroup: thread j takes the slots j, j + 256, j + 512, j + 768
WAVE = 64
F16_MAX = 65504.0


# ---- a tile's slots ----------------------------------------------------------------------------------------------------------------------------
def slot_of(dx, dy):
    """tile_slot (device_scene.h): the slot of the tile's pixel (dx, dy) -- 8 x 8 sub-blocks, four to a row of the tile."""
    return ((dy & 24) << 5) | ((dx & 24) << 3) | ((dy & 7) << 3) | (dx & 7)


def pixel_of(slot):
    """slot_pixel (chain_pass.h): (dx, dy) of a slot."""
    sub, l = slot >> 6, slot & 63
    return (sub & 3) * 8 + (l & 7), (sub >> 2) * 8 + (l >> 3)


def tile_grid(h, w):
    return (h + TILE - 1) // TILE, (w + TILE - 1) // TILE


def tile_by_slot(plane, ty, tx):
    """(values [1024], inside [1024]) of tile (ty, tx) of a [H][W] plane in slot order; slots outside the image hold 0 and are not inside."""
    h, w = plane.shape
    dx, dy = pixel_of(np.arange(SLOTS))
    x, y = tx * TILE + dx, ty * TILE + dy
    inside = (x < w) & (y < h)
    values = np.zeros(SLOTS, plane.dtype)
    values[inside] = plane[y[inside], x[inside]]
    return values, inside


def tile_reduce_order(values_by_slot, inside, wave_order=(0, 1, 2, 3)):
    """The fp32 sum of a tile's slots in exactly the order of chain_pass.h (tile_reduce): thread j adds its slots j, j + 256, j + 512, j + 768
    that are inside the image, in that order, starting from 0; the 64 lanes of a wave then run the butterfly v = v + v[lane ^ m] for
    m = 32 .. 1; one lane adds wave 0's partial and those of the waves 1, 2, 3 in that order (`wave_order`: another order, for tests)."""
    v = np.asarray(values_by_slot, np.float32).reshape(SLOTS // BLOCK, BLOCK)
    ins = np.asarray(inside, bool).reshape(SLOTS // BLOCK, BLOCK)
    with np.errstate(all="ignore"):
        acc = np.zeros(BLOCK, np.float32)
        for q in range(SLOTS // BLOCK):
            acc = np.where(ins[q], acc + v[q], acc)
        w = acc.reshape(BLOCK // WAVE, WAVE)
        lanes = np.arange(WAVE)
        m = WAVE // 2
        while m >= 1:
            w = w + w[:, lanes ^ m]
            m //= 2
        total = w[wave_order[0], 0]
        for o in wave_order[1:]:
            total = total + w[o, 0]
    return np.float32(total)


def tile_sums_in_order(plane):
    """[ty][tx] fp32: tile_reduce_order of every tile of a [H][W] plane."""
    ty, tx = tile_grid(*plane.shape)
    out = np.zeros((ty, tx), np.float32)
    for y in range(ty):
        for x in range(tx):
            out[y, x] = tile_reduce_order(*tile_by_slot(np.asarray(plane, np.float32), y, x))
    return out


# ---- chain counts and what a render leaves in the chains it does not reach ---------------------------------------------------------------------
def chain_counts(spp, first=0):
    """n_c of frames first .. first + spp - 1 (frame f belongs to chain f % 8)."""
    n = np.zeros(CHAINS, np.int64)
    for fr in range(first, first + spp):
        n[fr % CHAINS] += 1
    return n


def resolve(chains):
    """[3][H][W][3]: ((c0 + c1) + c2) + ... + c7 in fp32 -- what rene_download hands out."""
    with np.errstate(all="ignore"):
        acc = chains[0] + chains[1]
        for g in range(2, CHAINS):
            acc = acc + chains[g]
    return acc


def for_counts(chains, n_c):
    """A copy with the chains that hold no frames zeroed (every layer), as a render leaves them."""
    out = chains.copy()
    out[np.asarray(n_c) == 0] = 0.0
    return out


def for_tile_frames(chains, first, tile_frames):
    """A copy in which every tile holds the frames first .. first + tile_frames[ty][tx] - 1: the chains those frames do not reach are zeroed."""
    out = chains.copy()
    for (ty, tx), nt in np.ndenumerate(np.asarray(tile_frames)):
        empty = chain_counts(int(nt), first) == 0
        out[empty, :, ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE] = 0.0
    return out


def per_tile(h, w, tile_frames, make):
    """An [h][w] or [h][w][C] array whose tile (ty, tx) is cut from make(tile_frames[ty][tx]), an array of that shape computed for the whole
    image at that frame count (once per distinct count)."""
    cache, out = {}, None
    for (ty, tx), nt in np.ndenumerate(np.asarray(tile_frames)):
        nt = int(nt)
        if nt not in cache:
            cache[nt] = make(nt)
        if out is None:
            out = np.zeros_like(cache[nt])
        sl = (slice(ty * TILE, min(h, (ty + 1) * TILE)), slice(tx * TILE, min(w, (tx + 1) * TILE)))
        out[sl] = cache[nt][sl]
    return out


# ---- the edge film ------------------------------------------------------------------------------------------------------------------------------
# the counts the tie classes are built for: 12 frames from frame 3 leave chains of two frames (3 .. 6) and of one (7, 0, 1, 2)
TIE_FIRST, TIE_FRAMES = 3, 12
HUGE = np.float32(3e38)
# classes whose radiance is not finite, or overflows on the way: left out of the finite film
NON_FINITE = ("nan_one", "nan_all", "inf_one", "neg_inf_one", "inf_both", "overflow", "cap_inf")


def _classes(n_c):
    """name -> f(i) -> ([8][3] radiance of the class's i-th pixel, fill of the guide layers or None).  n_c: the chain counts the classes with equal
    MEANS are built for (C_c = n_c m_c is exact for the small n_c and the m_c used)."""
    nf = n_c.astype(np.float32)
    ramp = np.arange(1, CHAINS + 1, dtype=np.float32)

    def bg(i, lo=0.5, hi=1.5):  # a quiet pixel: means lo .. hi, different in every chain and channel
        r = np.random.default_rng(1000 + i)
        return (r.uniform(lo, hi, (CHAINS, 3)).astype(np.float32) * nf[:, None]).astype(np.float32)

    def rows(v):  # the same value in the three channels
        return np.repeat(np.asarray(v, np.float32)[:, None], 3, axis=1)

    def nan_one(i):
        c = bg(i)
        c[(2 + i) % CHAINS, i % 3] = np.nan
        return c, ("nan", (2 + i) % CHAINS)

    def nan_all(i):
        return np.full((CHAINS, 3), np.nan, np.float32), None

    def inf_one(i):
        c = bg(i)
        c[(5 + i) % CHAINS] = np.inf
        return c, ("inf", (3 + i) % CHAINS)

    def neg_inf_one(i):
        c = bg(i)
        c[(1 + i) % CHAINS, (i + 1) % 3] = -np.inf
        return c, None

    def inf_both(i):
        c = bg(i)
        c[i % CHAINS] = np.inf
        c[(i + 3) % CHAINS] = -np.inf
        return c, None

    def overflow(i):  # every chain finite, S0 and the sum of the luminances are not
        return np.full((CHAINS, 3), HUGE, np.float32), ("all", HUGE)

    def cap_inf(i):
        # chains 3 and 4 hold -3e38 and +3e38: they cancel in tot, which the chains after them make a small positive number, while
        # num = sum (2 r + 1 - k) l_c overflows to +inf: G = +inf, t = +inf, j = the cap.  (Chains 3 and 4 hold frames at every count used.)
        c = bg(i)
        c[3], c[4] = -HUGE, HUGE
        return c, None

    def negative(i):
        return -bg(i), None

    def neg_zero(i):
        return np.full((CHAINS, 3), -0.0, np.float32), ("all", np.float32(-0.0))

    def denormal(i):
        return rows(ramp * np.float32(1e-41) * np.float32(1 + i % 5)), ("ramp", np.float32(1e-41))

    def neg_denormal(i):
        return rows(-ramp * np.float32(3e-42)), ("ramp", np.float32(-1e-41))

    def firefly_one(i):
        c = bg(i)
        c[i % CHAINS] *= np.float32(1e4)
        return c, None

    def all_equal(i):  # equal means in chains of unequal length: every rank is the tie rule's
        return rows(nf * np.float32(0.75 + 0.25 * (i % 4))), None

    def tie_top(i):
        # five chains of mean 1, three of mean 50, the hot ones moving with the pixel: k = 8 gives G = 735 / 1240, t = 2.37, j = 2 -- ranks 2 .. 5
        # are kept, ONE of the three hot chains among them: which one is the tie rule's, and with chains of unequal length the output says so
        m = np.ones(CHAINS, np.float32)
        for o in (0, 3, 5):
            m[(i + o) % CHAINS] = 50.0
        return rows(nf * m), None

    def mild(i):  # one chain a few times brighter than the rest: small Gini coefficients, j = 0, 1 or 2 as the factor grows
        m = np.ones(CHAINS, np.float32)
        m[(4 + i) % CHAINS] = (3.0, 6.0, 6.5, 12.0)[i % 4]
        return rows(nf * m), None

    def zero(i):
        return np.zeros((CHAINS, 3), np.float32), None

    def zero_partial(i):  # ties between zero chains beside chains that are not zero
        m = np.zeros(CHAINS, np.float32)
        m[(3 + i) % CHAINS], m[(4 + i) % CHAINS] = 2.0, 0.5
        return rows(nf * m), None

    def clamp_pos(i):
        return rows(nf * np.float32(1e5 * (1 + i % 3))), None

    def clamp_neg(i):
        return rows(nf * np.float32(-7e4 * (1 + i % 3))), None

    def half_subnormal(i):  # means between the smallest half subnormal and the smallest normal half
        return rows(nf * np.float32(2.0 ** -(15 + i % 9) * 1.25)), None

    def half_tie(i):  # means exactly half-way between two halves (n_c m and their sums stay exact in fp32)
        m = (1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2048 + 1, 2048 + 3, 0.5 + 2.0 ** -12, 2.0 ** -14 + 2.0 ** -25)[i % 6]
        return rows(nf * np.float32(m)), None

    def cancel(i):  # luminances that cancel to tot == 0 with chains that are not zero
        m = np.zeros(CHAINS, np.float32)
        m[3], m[4] = 2.0, -2.0
        return rows(nf * m), None

    return dict(nan_one=nan_one, nan_all=nan_all, inf_one=inf_one, neg_inf_one=neg_inf_one, inf_both=inf_both, overflow=overflow, cap_inf=cap_inf,
                negative=negative, neg_zero=neg_zero, denormal=denormal, neg_denormal=neg_denormal, firefly_one=firefly_one, all_equal=all_equal,
                tie_top=tie_top, mild=mild, zero=zero, zero_partial=zero_partial, clamp_pos=clamp_pos, clamp_neg=clamp_neg,
                half_subnormal=half_subnormal, half_tie=half_tie, cancel=cancel)


def _guide_fill(c1, c2, fill, i):
    """What a class puts into the pixel's normal (c1) and albedo (c2) chain values [8][3]."""
    kind, v = fill
    if kind == "nan":
        c1[v, i % 3] = np.nan
    elif kind == "inf":
        c2[v, (i + 1) % 3] = np.inf
    elif kind == "all":
        c1[:], c2[:] = v, v
    elif kind == "ramp":
        r = (np.arange(1, CHAINS + 1, dtype=np.float32) * v)[:, None]
        c1[:], c2[:] = r, r


def edge_chains(h, w, seed=0):
    """(edge, finite, where): two films [8][3][h][w][3] fp32 and {class: [h][w] bool}.  A finite random background -- radiance uniform in
    [0, 4), three per cent of the chain entries times 1e4 as fireflies, unit normals, albedo in [0, 1] -- and over it the classes of _classes,
    each in three tiles: the rows of an interior tile (1, 1), the rows of the last tile column (ragged in x) and the columns of the last tile
    row (ragged in y).  `finite` carries the classes outside NON_FINITE only: every sum over it stays finite."""
    ty, tx = tile_grid(h, w)
    assert ty >= 3 and tx >= 3 and h % TILE and w % TILE, "the edge film wants an interior tile and ragged tiles on both sides"
    rng = np.random.default_rng(seed)
    film = np.zeros((CHAINS, 3, h, w, 3), np.float32)
    film[:, 0] = rng.uniform(0, 4, (CHAINS, h, w, 3)).astype(np.float32)
    film[:, 0][rng.random((CHAINS, h, w)) < 0.03] *= np.float32(1e4)
    nrm = rng.normal(size=(CHAINS, h, w, 3))
    film[:, 1] = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    film[:, 2] = rng.uniform(0, 1, (CHAINS, h, w, 3)).astype(np.float32)
    edge, finite = film, film.copy()
    classes = _classes(chain_counts(TIE_FRAMES, TIE_FIRST))
    assert len(classes) <= TILE
    where = {}
    for ci, (name, make) in enumerate(classes.items()):
        places = [(TILE + ci, x) for x in range(TILE, 2 * TILE)]                        # a row of the interior tile (1, 1)
        places += [(TILE + ci, x) for x in range((tx - 1) * TILE, w)]                   # a row of the tile (1, tx - 1), ragged in x
        places += [(y, TILE + ci) for y in range((ty - 1) * TILE, h)]                   # a column of the tile (ty - 1, 1), ragged in y
        mask = np.zeros((h, w), bool)
        for i, (y, x) in enumerate(places):
            c0, fill = make(i)
            targets = (edge,) if name in NON_FINITE else (edge, finite)
            for f in targets:
                f[:, 0, y, x] = c0
                if fill is not None:
                    c1, c2 = f[:, 1, y, x].copy(), f[:, 2, y, x].copy()
                    _guide_fill(c1, c2, fill, i)
                    f[:, 1, y, x], f[:, 2, y, x] = c1, c2
            mask[y, x] = True
        where[name] = mask
    return edge, finite, where


# ---- fp16 --------------------------------------------------------------------------------------------------------------------------------------
def half_ties():
    """The fp32 values around every rounding boundary of fp16: for every pair of adjacent finite halves the midpoint and its two fp32
    neighbours, both signs; 65504, the fp32 below 65520, 65520 (the first value that would round to infinity), 1e6, +-inf, NaN; 2^-24 (the
    smallest half), 2^-25 (half of it: a tie with zero) and its neighbours; +-0."""
    halves = np.arange(0, 0x7c00, dtype=np.uint16).view(np.float16).astype(np.float64)  # 0 .. 65504
    mid = ((halves[:-1] + halves[1:]) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (halves[:-1] + halves[1:]) / 2)  # exact in fp32
    around = np.concatenate([np.nextafter(mid, np.float32(-np.inf)), mid, np.nextafter(mid, np.float32(np.inf))])
    tiny = np.float32(2.0 ** -25)
    extra = np.array([65504.0, np.nextafter(np.float32(65520.0), np.float32(0)), 65520.0, 1e6, np.inf, 2.0 ** -24, tiny,
                      np.nextafter(tiny, np.float32(0)), np.nextafter(tiny, np.float32(1))], np.float32)
    pos = np.concatenate([around, extra])
    return np.concatenate([pos, -pos, np.array([np.nan, 0.0, -0.0], np.float32)]).astype(np.float32)


def is_half_tie(v):
    """Which fp32 values lie exactly half-way between two adjacent finite halves (the conversion has to pick the even one)."""
    a = np.abs(np.asarray(v, np.float64))
    ok = np.isfinite(a) & (a > 0) & (a < F16_MAX)
    _, e = np.frexp(np.where(ok, a, 1.0))               # a = m 2^e, 0.5 <= m < 1
    ulp = np.exp2(np.maximum(e - 1, -14) - 10.0)        # the spacing of the halves at a (subnormal halves: 2^-24)
    q = np.where(ok, a / (ulp / 2), 0.0)                # in units of half a spacing: a tie is an odd integer
    return ok & (q == np.floor(q)) & (np.floor(q) % 2 == 1)


def value_films(values, h, w):
    """The values spread over as many [h][w][3] fp32 films as they need, the last one padded with zeros."""
    per = h * w * 3
    n = (values.size + per - 1) // per
    flat = np.zeros(n * per, np.float32)
    flat[:values.size] = values
    return list(flat.reshape(n, h, w, 3))


def single_chain_load(film, scale, chain=0):
    """Chains [8][3][h][w][3] whose radiance holds scale * film in `chain` and zeros OF THE VALUE'S SIGN elsewhere -- so that the sums over the
    chains are scale * film bit for bit, a -0.0 included; the guide layers are zero."""
    h, w, _ = film.shape
    out = np.zeros((CHAINS, 3, h, w, 3), np.float32)
    out[:, 0] = np.copysign(np.float32(0), film)
    with np.errstate(all="ignore"):
        out[chain, 0] = film * np.float32(scale)
    return out


# ---- comparing bits ----------------------------------------------------------------------------------------------------------------------------
def differing(got, want):
    """Boolean array of the elements that differ under the rule of the tests called "bit for bit": where `want` is a NaN `got` must be one
    (payload and sign are free: x86 and the device produce different default NaNs); everywhere else the bits must be equal (-0.0 != 0.0)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bits = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    nan = np.isnan(want)
    return np.where(nan, ~np.isnan(got), np.ascontiguousarray(got).view(bits) != np.ascontiguousarray(want).view(bits))
