"""CPU: the helper of the chain-pass edge tests (tests/chain_reference.py) -- that tile_reduce_order restates an ORDER and agrees with a plain
sum, that its slot map is a bijection, and that the crafted films contain every class of input tests/test_gpu_chain_edges.py claims to put on
the device.  The class conditions are asserted here, on the numpy restatements alone, so that no GPU test can pass by leaving a class out."""
import numpy as np
import pytest

import chain_reference as cr
import features_reference as fr
import noise_reference as nr
import robust_reference as rr

EDGE_H, EDGE_W = 130, 161  # the film of the GPU tests: 5 x 6 tiles, the last column 1 pixel wide, the last row 2 pixels high
FIRST = 3
COUNTS = (12, 5, 16)       # chains of unequal length, three empty chains, equal chains


@pytest.fixture(scope="module")
def films():
    return cr.edge_chains(EDGE_H, EDGE_W, seed=0)


def test_slot_map_is_tile_slots_inverse():
    seen = np.zeros(cr.SLOTS, int)
    for dy in range(cr.TILE):
        for dx in range(cr.TILE):
            s = cr.slot_of(dx, dy)
            assert 0 <= s < cr.SLOTS and cr.pixel_of(s) == (dx, dy)
            seen[s] += 1
    assert (seen == 1).all()
    # eight consecutive pixels of a row are eight consecutive slots, an 8 x 8 sub-block is 64 of them (device_scene.h)
    assert [cr.slot_of(dx, 0) for dx in range(9)] == list(range(8)) + [64] and cr.slot_of(0, 1) == 8 and cr.slot_of(0, 8) == 256
    # tile_by_slot: the slots of a ragged tile outside the image are not inside, and the values arrive in slot order
    plane = np.arange(40 * 70, dtype=np.float32).reshape(40, 70)
    v, inside = cr.tile_by_slot(plane, 1, 2)
    assert int(inside.sum()) == 8 * 6
    for s in range(cr.SLOTS):
        dx, dy = cr.pixel_of(s)
        assert inside[s] == (64 + dx < 70 and 32 + dy < 40)
        if inside[s]:
            assert v[s] == plane[32 + dy, 64 + dx]


def test_tile_reduce_order_restates_an_order():
    """Wave w's threads are 64 w .. 64 w + 63.  Partials 1, 2^-24, 2^-24, 0: in wave order (1 + 2^-24) rounds back to 1 twice; with the waves
    1 and 2 first, 2^-24 + 2^-24 = 2^-23 survives the addition of 1."""
    v = np.zeros(cr.SLOTS, np.float32)
    v[0], v[64 + 5 + 256], v[128 + 17 + 768] = 1.0, 2.0 ** -24, 2.0 ** -24
    inside = np.ones(cr.SLOTS, bool)
    assert cr.tile_reduce_order(v, inside) == np.float32(1.0)
    swapped = cr.tile_reduce_order(v, inside, wave_order=(1, 2, 0, 3))
    assert swapped == np.float32(1.0 + 2.0 ** -23) and swapped.view(np.uint32) != np.float32(1.0).view(np.uint32)
    # the same input with the two waves' SLOTS exchanged instead of their partials: the order is a property of the slots
    w = v.copy()
    w[0], w[64 + 5 + 256] = v[64 + 5 + 256], v[0]
    assert cr.tile_reduce_order(w, inside) == np.float32(1.0)       # (2^-24 + 1) + 2^-24: each addition rounds to even
    w = np.zeros(cr.SLOTS, np.float32)
    w[128], w[0], w[64] = 1.0, 2.0 ** -24, 2.0 ** -24                # waves 0 and 1 hold the small ones, wave 2 the 1
    assert cr.tile_reduce_order(w, inside) == np.float32(1.0 + 2.0 ** -23)
    # a thread's own slots: j, j + 256, j + 512, j + 768 in that order, those outside the image skipped
    t = np.zeros(cr.SLOTS, np.float32)
    t[7], t[7 + 256], t[7 + 512] = 1.0, 2.0 ** -24, 2.0 ** -24
    assert cr.tile_reduce_order(t, inside) == np.float32(1.0)
    t[7], t[7 + 512] = t[7 + 512], t[7]
    assert cr.tile_reduce_order(t, inside) == np.float32(1.0 + 2.0 ** -23)
    out = inside.copy()
    out[7 + 512] = False                                              # the 1 is outside the image: it does not count
    assert cr.tile_reduce_order(t, out) == np.float32(2.0 ** -23)
    # the butterfly: lane l adds lane l ^ 32 first -- (1 + 2^-24) + 2^-24 = 1 where the two small ones meet the 1 one after the other ...
    b = np.zeros(cr.SLOTS, np.float32)
    b[0], b[32], b[16] = 1.0, 2.0 ** -24, 2.0 ** -24
    assert cr.tile_reduce_order(b, inside) == np.float32(1.0)
    b[32], b[48] = 0.0, 2.0 ** -24                                    # ... and 1 + (2^-24 + 2^-24) where they meet each other first
    assert cr.tile_reduce_order(b, inside) == np.float32(1.0 + 2.0 ** -23)


def _spread(plane):
    """max over tiles of |ordered fp32 sum - fp64 sum of the same pixels| / (|fp64| + the largest tile's value): the measure of the spreads
    recorded in tests/test_gpu_robust.py and tests/test_gpu_noise.py."""
    got = cr.tile_sums_in_order(plane).astype(np.float64)
    want = fr.tile_sums(np.asarray(plane, np.float32), np.float64)
    return float((np.abs(got - want) / (np.abs(want) + np.abs(want).max())).max())


def test_tile_reduce_order_agrees_with_an_fp64_sum(films):
    """On the planes the GPU tests sum -- the finite film's luminances and variances -- the ordered fp32 sum stays within the fp32-vs-fp64
    spread recorded for the restatements' own sums: 4.8e-8 (the robust resolve's) and 8.2e-8 (the noise estimate's)."""
    _, finite, _ = films
    n_c = cr.chain_counts(12, FIRST)
    c = cr.for_counts(finite, n_c)[:, 0]
    rob = rr.resolve(c, n_c, dtype=np.float32)
    l, var = nr.pixel_stats(c, n_c, np.float32)
    figures = {k: _spread(p) for k, p in (("lum_plain", rob["lum_plain"]), ("lum_robust", rob["lum_robust"]), ("noise l", l), ("noise var", var))}
    print("tile_reduce_order against fp64, max over tiles of |diff| / (|value| + largest tile):", {k: f"{v:.3g}" for k, v in figures.items()})
    assert figures["lum_plain"] <= 4.8e-8 and figures["lum_robust"] <= 4.8e-8
    assert figures["noise l"] <= 8.2e-8 and figures["noise var"] <= 8.2e-8


def test_every_class_lies_in_three_kinds_of_tile(films):
    edge, finite, where = films
    ty, tx = cr.tile_grid(EDGE_H, EDGE_W)
    assert (ty, tx) == (5, 6) and EDGE_W - (tx - 1) * 32 == 1 and EDGE_H - (ty - 1) * 32 == 2
    for name, mask in where.items():
        tiles = {(y // 32, x // 32) for y, x in zip(*np.nonzero(mask))}
        assert (1, 1) in tiles and (1, tx - 1) in tiles and (ty - 1, 1) in tiles, name
        assert int(mask.sum()) >= 32 + 1 + 2, name
    assert np.isfinite(finite).all() and not np.isfinite(edge).all()
    assert float(np.abs(finite).max()) < 1e6  # no sum over it overflows
    out = np.logical_or.reduce([where[n] for n in cr.NON_FINITE])
    assert np.array_equal(edge[:, :, ~out].view(np.uint32), finite[:, :, ~out].view(np.uint32))  # elsewhere the two films are the same
    # the background is what the issue asks for: radiance in [0, 4) with a few per cent of fireflies, unit normals, albedo in [0, 1]
    bgd = ~np.logical_or.reduce(list(where.values()))
    rad = finite[:, 0][:, bgd]
    fly = (rad > 4).any(axis=-1).mean()
    assert 0.01 < fly < 0.06 and rad.min() >= 0 and np.allclose(np.linalg.norm(finite[:, 1][:, bgd], axis=-1), 1, atol=1e-6)
    assert finite[:, 2][:, bgd].min() >= 0 and finite[:, 2][:, bgd].max() <= 1


@pytest.mark.parametrize("spp", COUNTS)
def test_the_edge_film_meets_every_class_of_the_robust_resolve(films, spp):
    """The cap: at 12, 5 and 16 frames from frame 3 the fp32 restatement of the robust resolve, on the edge film, meets every j the count
    allows (0 .. min(3, (k - 1) / 2): five frames fill five chains, whose cap is 2) and at least 8 pixels of every edge class."""
    edge, _, where = films
    n_c = cr.chain_counts(spp, FIRST)
    c = cr.for_counts(edge, n_c)[:, 0]
    k = int((n_c > 0).sum())
    out = rr.resolve(c, n_c, dtype=np.float32)
    img, j = out["image"], out["j"]
    assert set(np.unique(j)) == set(range(min(3, (k - 1) // 2) + 1)), np.unique(j)
    full = [g for g in range(8) if n_c[g] > 0]
    with np.errstate(all="ignore"):
        means = np.stack([c[g] / np.float32(n_c[g]) for g in full])
        l = rr.lum(means, np.float32)                                     # [k][H][W]
        tot = l[0].copy()
        for a in range(1, k):
            tot = tot + l[a]
    eq = (l[:, None] == l[None, :]) & ~np.eye(k, dtype=bool)[:, :, None, None]
    tied = eq.any(axis=(0, 1)) & (l != 0).any(axis=0)                     # ties between chain luminances, other than all-zero pixels
    lengths = np.asarray([n_c[g] for g in full])
    unequal = (eq & (lengths[:, None] != lengths[None, :])[:, :, None, None]).any(axis=(0, 1))
    tiny = np.float32(np.finfo(np.float32).tiny)
    figures = {
        "NaN output": int(np.isnan(img).any(axis=-1).sum()),
        "infinite output": int(np.isinf(img).any(axis=-1).sum()),
        "tied luminances": int(tied.sum()),
        "tied, j > 0": int((tied & (j > 0)).sum()),
        "denormal means": int(((np.abs(means) > 0) & (np.abs(means) < tiny)).any(axis=(0, -1)).sum()),
        "negative luminance": int((out["lum_plain"] < 0).sum()),
        "NaN tot (G = 0)": int(np.isnan(tot).sum()),
        "t = +inf (j = the cap)": int((where["cap_inf"] & (j == min(3, (k - 1) // 2))).sum()),
        "S0 overflows": int((np.isinf(out["plain"]).any(axis=-1) & np.isfinite(c).all(axis=(0, -1))).sum()),
    }
    if k == 8:  # (an empty chain holds +0.0, and -0.0 + 0.0 is +0.0: the sum keeps its sign only where every chain holds frames)
        figures["-0.0 sums"] = int(np.signbit(cr.resolve(cr.for_counts(edge, n_c))[0][where["neg_zero"]]).all(axis=-1).sum())
    if spp == 12:  # the only count with chains of unequal length: there the tie rule decides between chains that weigh differently
        figures["tied between chains of unequal length, j > 0"] = int((unequal & (j > 0)).sum())
    print(f"{spp} frames from {FIRST} (k = {k}): j histogram {np.bincount(j.ravel(), minlength=4).tolist()};", figures)
    for name, n in figures.items():
        assert n >= 8, (name, n)
    if spp == 12:
        # ... and says so in the output: ranking the tied chains the other way round (the higher chain first) gives other pixels
        flipped = rr.resolve(c[::-1], n_c[::-1], dtype=np.float32)["image"]
        changed = cr.differing(flipped, img).any(axis=-1) & where["tie_top"]
        print(f"pixels of the tie class whose output the tie rule decides: {int(changed.sum())}")
        assert int(changed.sum()) >= 8


def test_the_fp16_sweep_meets_every_class():
    """The cap of the fp16 converter's sweep: through the restatement, the films of half_ties() give COLOR == v bit for bit, and their fp16
    tensor holds clamped values of both signs, NaNs, subnormal halves and at least 60 000 exact ties."""
    v = cr.half_ties()
    films = cr.value_films(v, 64, 512)
    assert len(films) == 2 and v.dtype == np.float32
    ones = np.ones(8, np.int64)
    n_tie = n_sub = n_nan = n_hi = n_lo = 0
    for film in films:
        for scale, bit in ((8, fr.COLOR), (4, fr.HALF_A)):
            chains = cr.single_chain_load(film, scale)
            got = fr.features(chains[:, 0], ones)[bit]
            assert not cr.differing(got, film).any()          # the value reaches the converter bit for bit, -0.0 included
        h = fr.to_f16(film)
        n_tie += int(cr.is_half_tie(film).sum())
        n_sub += int(((np.abs(h) > 0) & (np.abs(h) < np.float16(2.0 ** -14))).sum())
        n_nan += int(np.isnan(h).sum())
        n_hi += int(((film > 65504) & (h == np.float16(65504))).sum())
        n_lo += int(((film < -65504) & (h == np.float16(-65504))).sum())
    print(f"half_ties(): {v.size} values in {len(films)} films; exact ties {n_tie}, subnormal halves {n_sub}, NaN {n_nan}, clamped {n_hi} / {n_lo}")
    assert n_tie >= 60000 and n_sub >= 1000 and n_nan >= 1 and n_hi >= 3 and n_lo >= 3
    # is_half_tie on values whose answer is known: the midpoint of 1 and its successor, its fp32 neighbours, and a half itself
    mid = np.float32(1 + 2.0 ** -11)
    assert cr.is_half_tie(np.array([mid, np.nextafter(mid, np.float32(2)), np.nextafter(mid, np.float32(0)), 1.0, 2.0 ** -25, 65520.0], np.float32)).tolist() == \
        [True, False, False, False, True, False]
    # ties round to even: 1 + 2^-11 -> 1 (even mantissa), 1 + 3 2^-11 -> 1 + 2^-9
    assert fr.to_f16(np.float32(1 + 2.0 ** -11)) == np.float16(1) and fr.to_f16(np.float32(1 + 3 * 2.0 ** -11)) == np.float16(1 + 2.0 ** -9)


def test_the_edge_film_meets_every_class_of_the_feature_export(films):
    """... and the edge film's own fp16 tensor: clamped values of both signs, NaNs, subnormal halves, ties, -0.0."""
    edge, _, where = films
    n_c = cr.chain_counts(12, FIRST)
    c = cr.for_counts(edge, n_c)
    s = cr.resolve(c)
    t32 = fr.tensor(fr.features(c[:, 0], n_c, s[1], s[2]), fr.ALL)
    t16 = fr.to_f16(t32)
    figures = {"clamped high": int(((t32 > 65504) & (t16 == np.float16(65504))).sum()), "clamped low": int(((t32 < -65504) & (t16 == np.float16(-65504))).sum()),
               "NaN": int(np.isnan(t16).sum()), "subnormal halves": int(((np.abs(t16) > 0) & (np.abs(t16) < np.float16(2.0 ** -14))).sum()),
               "exact ties": int(cr.is_half_tie(t32).sum()), "-0.0": int((np.signbit(t16) & (t16 == 0)).sum()),
               "fp32 denormals": int(((np.abs(t32) > 0) & (np.abs(t32) < np.finfo(np.float32).tiny)).sum())}
    print("the edge film's feature tensor:", figures)
    for name, n in figures.items():
        assert n >= 8, (name, n)


def test_load_chains_is_exported_and_refuses_null(hip_lib):
    """The probe's host surface without a GPU: the symbol, its place in the ABI list, and the NULL refusal with a message."""
    import ctypes as C
    from rene_amd import abi
    assert "rene_load_chains" in abi.EXPORTED_SYMBOLS and hip_lib.rene_abi_version() == abi.ABI_VERSION == 7  # an added symbol: no version change
    buf = np.zeros(8, np.float32)
    assert hip_lib.rene_load_chains(None, buf.ctypes.data_as(C.c_void_p), buf.size, 0, 8, None, 0) == -1
    assert b"rene_load_chains" in hip_lib.rene_last_error()
