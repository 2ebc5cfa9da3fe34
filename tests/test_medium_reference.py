"""CPU: the fp64 media reference of tests/medium_reference.py against closed forms it does not itself use; the set-aside caps, which are
conditions on the inputs that the reference alone has to meet; and the oracle (medium_eval) through the same check() as the device, on the
inputs the GPU test uses.  The oracle keeps denormals: its flush samples sit on the IEEE answer.  The same for the transmittance walks:
walk() against slab products, chords in closed form and the `tmin` rule written out by hand, the set-aside cap per scene and start medium, and
the oracle's walk probe (oracle_transmittance) through walk_check(), query counts exact."""
import numpy as np
import pytest

import bsdf_reference as br
import medium_reference as mr


def _hg(mu, g):
    """Henyey-Greenstein in pbrt's sign convention, written out here on its own."""
    d = 1 + g * g + 2 * g * mu
    return (1 - g * g) / (4 * np.pi * d ** 1.5)


# ---- the seeds and the rows ----------------------------------------------------------------------------------------------------------------------------------
def test_edge_seeds_draw_what_their_rows_say():
    seeds = mr._edge_seeds()
    f32 = lambda w: (w >> 8) * 2.0 ** -24
    for c in range(3):
        d = mr.draws_of(seeds[f"distance draw 0, channel {c}"], 2)
        assert d[0] % 3 == c and f32(d[1]) == 0.0
        d = mr.draws_of(seeds[f"distance draw 1 - 2^-24, channel {c}"], 2)
        assert d[0] % 3 == c and f32(d[1]) == 1.0 - 2.0 ** -24
    assert mr.draws_of(seeds["channel draw 0xFFFFFFFF"], 1)[0] == 0xFFFFFFFF
    assert f32(mr.draws_of(seeds["u0 = 0"], 3)[2]) == 0.0 and f32(mr.draws_of(seeds["u0 = 1 - 2^-24"], 3)[2]) == 1.0 - 2.0 ** -24
    for name, v in (("0", 0.0), ("1/4", 0.25), ("1/2", 0.5), ("3/4", 0.75)):
        assert f32(mr.draws_of(seeds[f"u1 = {name}"], 4)[3]) == v
    # the generalisation agrees with bsdf_reference's two special cases
    assert mr.seed_with_draw(1, range(0, 256)) == br.seed_with(first=range(0, 256))
    assert mr.seed_with_draw(2, range(0, 256)) == br.seed_with(second=range(0, 256))


def test_the_catalogue_holds_what_it_says():
    g = [mr.MEDIA[c][2] for c in mr.CASES if c.startswith("grey")]
    below, at = np.nextafter(np.float32(1e-3), np.float32(0)), np.float32(1e-3)
    for s in (1.0, -1.0):
        for v in (0.3, 0.7, 0.9, 0.99, 0.999, float(below), float(at), 1.001e-3):
            assert s * v in g
    assert 0.0 in g and below < at and np.float32(1.001e-3) > at
    for name in mr.SIGMAS:
        if name != "grey":
            assert f"{name} g=0.0" in mr.MEDIA and f"{name} g=0.7" in mr.MEDIA
    assert "dense g=-0.99" in mr.MEDIA
    total = lambda name: np.float32(mr.SIGMAS[name][0]) + np.float32(mr.SIGMAS[name][1])
    np.testing.assert_allclose(total("grey"), [1, 1, 1])
    np.testing.assert_allclose(total("chromatic"), [0.05, 1, 20], rtol=1e-6)
    np.testing.assert_allclose(total("dense"), [40, 60, 90])
    assert total("one channel empty")[1] == 0 and (np.float32(mr.SIGMAS["sigma_s = 0"][1]) == 0).all() and (np.float32(mr.SIGMAS["sigma_a = 0"][0]) == 0).all()
    S = mr.shared_scene()
    assert len(S.scene.mediums) == len(mr.CASES) and S.index["vacuum"] == 0
    I = mr.uniform_set("grey g=0.0")
    length = np.linalg.norm(I.rd.astype(np.float64), axis=1)
    assert len(I.t_max) == mr.N_UNIFORM and length.min() < 0.2 and length.max() > 5 and I.t_max.min() < 0.02 and I.t_max.max() > 6
    # the dense medium's t_max <= 3 crosses both ends of the flush zone in tr
    tau = 90.0 * 3.0
    assert tau > 103.97 and np.exp(-87.34) < 1.0001 * mr.FLT_MIN < np.exp(-87.33) and np.exp(-103.98) < mr.DENORM_MIN < np.exp(-103.27)


def test_decisions_are_recorded():
    ref = mr.reference("chromatic g=0.7", "uniform")
    for name in ("channel", "t<t_max", "pdf==0", "|g|<1e-3", "|x|>|y|"):
        assert ref.dec.items[name][0].all(), name
    assert set(np.unique(ref.dec.items["channel"][1])) == {0, 1, 2}
    assert 0.2 < ref.dec.items["t<t_max"][1].mean() < 0.8 and not ref.dec.items["pdf==0"][1].any()
    assert not ref.dec.items["|g|<1e-3"][1].any() and 0.3 < ref.dec.items["|x|>|y|"][1].mean() < 0.7
    assert (ref.draws == 4).all()
    for case in mr.CASES:
        if case.startswith("grey"):
            iso = mr.reference(case, "edge").dec.items["|g|<1e-3"][1].all()
            assert iso == (abs(np.float32(mr.MEDIA[case][2])) < np.float32(1e-3)), case
    assert not mr.reference("grey g=0.0010000000474974513", "edge").dec.items["|g|<1e-3"][1].any()  # 1e-3 itself takes the anisotropic branch
    tie = mr.edge_set("grey g=0.7").names.index("|wo.x| == |wo.y|")
    assert not mr.reference("grey g=0.7", "edge").dec.items["|x|>|y|"][1][tie]                      # a tie takes the second form


# ---- closed forms the reference does not itself use --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", mr.G_VALUES)
def test_the_phase_function_integrates_to_one(g):
    """By quadrature over mu = cos: a substitution that follows the peak (mu = -sign(g) + ... is resolved by a grid that is geometric towards it)."""
    g = float(np.float32(g))
    e = np.linspace(-16, 0, 400001)
    x = np.concatenate([[0.0], 2.0 * 10.0 ** e])          # the distance from the peak's end of [-1, 1]
    mu = (-1.0 + x) if g >= 0 else (1.0 - x)
    n = len(mu)
    wo = np.tile(np.float64([[0.0, 0.0, 1.0]]), (n, 1))
    wi = np.stack([np.sqrt(np.fmax(1 - mu * mu, 0)), np.zeros(n), mu], -1)
    m = mr.Medium(*mr.SIGMAS["grey"], g)
    P = mr._pattern(-1)
    phase = mr._core(m, wo, np.ones(n), wo, wi, np.zeros(n, np.uint64), P, "ieee").phase
    np.testing.assert_allclose(phase, _hg(mu, g), rtol=1e-6)  # fp32(pi) is pi to 3e-8; wi is a unit vector to 1e-16, amplified at the peak of 0.999
    total = 2 * np.pi * np.trapezoid(phase, x)
    assert total == pytest.approx(1.0, abs=2e-5)


@pytest.mark.parametrize("case", [c for c in mr.CASES if c.startswith("grey")])
def test_the_mean_sampled_cosine_is_minus_g(case):
    g = mr.MEDIA[case][2]
    n = 1 << 16
    rng = np.random.default_rng(3)
    wo = br._sphere(rng, n)
    r = mr.evaluate(mr.medium_of(case), np.ones((n, 3)), np.ones(n), wo, wo, rng.integers(0, 1 << 32, n, dtype=np.uint64))
    wo = wo.astype(np.float32).astype(np.float64)
    c = (r.p * wo).sum(-1)
    assert c.mean() == pytest.approx(-g, abs=5e-3)
    np.testing.assert_allclose(np.linalg.norm(r.p, axis=1), 1.0, atol=1e-6)      # wo is a unit vector to fp32's 6e-8
    np.testing.assert_allclose(c, r.cos_t, atol=1e-6)                              # the frame is orthogonal to wo
    # and it is distributed as 2 pi hg(cos): the sampled cosines' CDF against the closed form's
    grid = np.linspace(-1, 1, 41)[1:-1]  # the ends themselves hold the peak of |g| = 0.999, to within the 6e-8 by which |wo| is not 1
    # the integral of 2 pi hg from -1 to mu, in closed form: (1 - g^2) / (2 g) (1 / |1 - g| - 1 / sqrt(1 + g^2 + 2 g mu)); (mu + 1) / 2 at g = 0
    cdf = (grid + 1) / 2 if g == 0 else (1 - g * g) / (2 * g) * (1 / abs(1 - g) - 1 / np.sqrt(1 + g * g + 2 * g * grid))
    np.testing.assert_allclose(np.searchsorted(np.sort(c), grid) / n, cdf, atol=8e-3)  # 4 sigma of a binomial share at 65 536


@pytest.mark.parametrize("case", ["grey g=0.0", "chromatic g=0.0", "one channel empty g=0.0", "dense g=0.0", "thin g=0.0", "defaults g=0.0"])
def test_the_sampled_fraction_and_the_weights_expectation(case):
    """P(sampled) is the channel mean of 1 - exp(-tau), and the unsampled weight tr / mean(tr) times the probability mean(tr) of staying unsampled
    is Beer-Lambert per channel: E[weight 1{unsampled}] = exp(-tau_c), the estimator's point."""
    n = 1 << 16
    rng = np.random.default_rng(5)
    m = mr.medium_of(case)
    st = m.sigma_a + m.sigma_s
    scale = 1.0 / max(st.max(), 1e-30)
    rd = np.tile(np.float32([[0.0, 0.0, 2.0]]), (n, 1))
    t_max = np.full(n, np.float32(0.4 * scale))
    wo = np.tile(np.float64([[0.0, 0.0, 1.0]]), (n, 1))
    r = mr.evaluate(m, rd, t_max, wo, wo, rng.integers(0, 1 << 32, n, dtype=np.uint64))
    tau = st * 2.0 * float(t_max[0])
    assert r.sampled.mean() == pytest.approx((1 - np.exp(-tau)).mean(), abs=8e-3)
    unsampled = np.where(r.sampled[:, None], 0.0, r.weight).mean(0)
    np.testing.assert_allclose(unsampled, np.exp(-tau), atol=1.5e-2)
    np.testing.assert_allclose(r.tr, np.tile(np.exp(-tau), (n, 1)), rtol=1e-12)
    assert (r.weight >= 0).all() and (r.weight <= 3 * (1 + 1e-12)).all()
    np.testing.assert_allclose(np.linalg.norm(r.position, axis=1)[~r.sampled], 2.0 * float(t_max[0]), rtol=1e-12)


def test_the_empty_channel_at_a_zero_draw_ends_at_t_max():
    """dist = -ln(1) / 0 = -0 / 0 = NaN; `t < t_max` is false and min(NaN, t_max) is t_max (medium.rs:113-117)."""
    case = "one channel empty g=0.0"
    I, ref = mr.edge_set(case), mr.reference(case, "edge")
    i = I.names.index("distance draw 0, channel 1")
    assert not ref.sampled[i] and not ref.aside["position"][i] and not ref.aside["weight"][i]
    np.testing.assert_allclose(ref.position[i], I.t_max[i].astype(np.float64) * I.rd[i].astype(np.float64), rtol=1e-15)
    assert np.isfinite(ref.weight[i]).all() and ref.weight[i, 1] == pytest.approx(1.0 / ((ref.s_tr[i].sum()) / 3.0))


def test_a_real_defect_is_far_outside_the_allowance():
    """For scale: the density without sigma_t, the phase with the other sign, and tr without |rd|, against the allowance of the same samples."""
    case = "chromatic g=0.7"
    I, ref = mr.uniform_set(case), mr.reference(case, "uniform")
    m = mr.medium_of(case)
    st = m.sigma_a + m.sigma_s
    s = ref.sampled & ~ref.aside["weight"] & ~ref.flush
    wrong = np.exp(-ref.x) * m.sigma_s / (np.exp(-ref.x).sum(-1) / 3.0)[:, None]
    assert np.median((np.abs(wrong - ref.weight) / ref.allow["weight"]).max(-1)[s]) > 1e3
    cos = (I.wo.astype(np.float64) * I.wi.astype(np.float64)).sum(-1)
    assert np.median(np.abs(_hg(-cos, m.g) - ref.phase) / ref.allow["phase"]) > 1e3
    wrong = np.exp(-st * I.t_max.astype(np.float64)[:, None])
    lit = (ref.tr > 1e-3).all(-1)
    assert np.median((np.abs(wrong - ref.tr) / ref.allow["tr"]).max(-1)[lit]) > 1e3


# ---- the caps and the oracle -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mr.CASES)
def test_the_inputs_stay_within_the_set_aside_caps(case):
    for which in mr.SETS:
        shares = mr.aside_shares(case, which)
        ref = mr.reference(case, which)
        print(f"{case} {which}: set aside " + ", ".join(f"{q} {100 * s:.1f} %" for q, (s, _) in shares.items()) + f"; flush {int(ref.flush.sum())}")
        cap = 0.0 if which == "edge" else mr.SET_ASIDE_CAP
        for q, (share, rows) in shares.items():
            assert share <= cap, (case, which, q, share, [mr.edge_set(case).names[i] for i in rows] if which == "edge" else rows[:8])
        assert which == "edge" or ref.flush.mean() <= 0.05, (case, which)  # its own class, and a small one: the other samples carry the comparison


def test_every_exemption_names_rows_of_the_edge_set():
    for prefix, (quantities, cases, reason) in mr.EDGE_EXEMPT.items():
        assert set(quantities) <= set(mr.QUANTITIES) and reason and set(cases) <= set(mr.CASES)
        for case in cases:
            I, ref = mr.edge_set(case), mr.reference(case, "edge")
            hit = [i for i, k in enumerate(I.names) if k.startswith(prefix)]
            assert hit and all(ref.aside[q][i] for q in quantities for i in hit), (prefix, case)  # an exemption that nothing needs is dropped


def test_the_flush_zone_is_reached_and_is_a_class_of_its_own():
    ref = mr.reference("chromatic g=0.0", "uniform")
    assert ref.flush.sum() >= 8 and ref.alt is not None
    differ = (np.abs(ref.weight - ref.alt.weight) > ref.allow["weight"] + ref.alt.allow["weight"]).any(-1)
    assert not differ[~ref.flush].any()  # outside the zone the two answers are one
    for case in mr.CASES:  # pdf >= density_c / 3 with the drawn channel's optical depth under 16.6: pdf never flushes, `pdf == 0` is never taken
        for which in mr.SETS:
            r = mr.reference(case, which)
            if not mr.medium_of(case).vacuum:
                assert (r.s_pdf > 2.0 ** -60).all() and not r.dec.items["pdf==0"][1].any(), (case, which)


@pytest.mark.parametrize("case", mr.CASES)
def test_the_oracle_stays_within_the_allowance(case, oracle_mod):
    for which in mr.SETS:
        rows = mr.oracle_rows(oracle_mod, case, which)
        result, classes, flush = mr.check(rows, case, which)
        I = mr.input_set(case, which)
        name = lambda bad: [I.names[i] for i in np.nonzero(bad)[0]] if I.names else np.nonzero(bad)[0][:8]
        print(f"{case} {which}: oracle error / allowance " + ", ".join(f"{q} {r:.2f}" for q, (r, _) in result.items()) + f"; flush {flush}")
        for q, (_, bad) in result.items():
            assert not bad.any(), (case, which, q, int(bad.sum()), name(bad), rows[bad][:3])
        for k, bad in classes.items():
            assert not bad.any(), (case, which, k, int(bad.sum()), name(bad), rows[bad][:3])
        off = mr.oracle_flush_on_ieee(rows, case, which)
        assert not off.any(), (case, which, "flush samples off the IEEE answer", name(off))


# ---- the walks -------------------------------------------------------------------------------------------------------------------------------------------------
def _sigma(D, k):
    return D.sigma_t[k]


def test_slab_walks_are_the_product_of_beer_lambert_factors():
    """Every ray of `slabs` crosses the five boundaries: the path in each slab is 1 / cos(theta) long whatever |rd| is.  Written per region, by
    hand: the start medium to z = 1, 1 in [1, 2], 2 in [2, 3], the vacuum in [3, 4], the vacuum again in [4, 5] (the flipped, unswapped
    boundary at z = 4: medium 3 was meant), medium 4 from z = 5 to the terminator at z = 6 -- or nothing, behind z = 5, for a ray that misses."""
    D = mr.walk_description("slabs")
    for start in range(5):
        o, d = (v.astype(np.float64) for v in mr.walk_rays("slabs", start))
        sec = np.linalg.norm(d, axis=1) / d[:, 2]
        tau = sum(_sigma(D, k) if k else 0.0 for k in (start, 1, 2)) * sec[:, None]
        ref0, ref1 = mr.walk_reference("slabs", start, False), mr.walk_reference("slabs", start, True)
        x6 = o[:, 0] + 6.0 * d[:, 0] / d[:, 2]
        # tr_emit returns tr times the radiance at the light without the factor of the segment that ends on it (lib.rs:447-451 come before 455-458):
        # medium 4, from z = 5 to the light at z = 6, never attenuates.  Pinned like the other quirks
        behind = np.exp(-tau)
        miss, matte, facing, averted = x6 < -10, (x6 > -10) & (x6 < 0), (x6 > 0) & (x6 < 10), x6 > 10
        assert min(miss.sum(), matte.sum(), facing.sum(), averted.sum()) > 150
        # a miss leaves z = 5 in medium 4 and never meets another surface: no factor for it (lib.rs:391-392)
        np.testing.assert_allclose(ref0.tr[miss], np.exp(-tau)[miss], rtol=1e-12)
        assert (ref0.tr[~miss] == 0).all() and (ref1.tr[miss | matte | averted] == 0).all()
        np.testing.assert_allclose(ref1.tr[facing], (behind * np.float64(mr._L))[facing], rtol=1e-12)
        assert (ref0.queries == 6).all() and (ref1.queries == 6).all()
        assert (ref0.ended[miss] == 0).all() and (ref0.ended[~miss] == 1).all()
        assert (ref1.ended[matte] == 1).all() and (ref1.ended[facing] == 2).all() and (ref1.ended[averted] == 3).all()
    lengths = np.unique(np.round(np.linalg.norm(mr.walk_rays("slabs", 0)[1].astype(np.float64), axis=1), 5))
    np.testing.assert_allclose(lengths, [0.5, 1.0, 2.0])
    angle = np.degrees(np.arccos(1 / sec))
    assert angle.min() < 5 and angle.max() > 75


def test_the_thin_pairs_skip_exactly_within_tmin():
    D = mr.walk_description("thin")
    o, d = (v.astype(np.float64) for v in mr.walk_rays("thin", 0))
    ref = mr.walk_reference("thin", 0, False)
    s1, s2 = _sigma(D, 1), _sigma(D, 2)
    gap1, gap2 = float(np.float32(1.0005)) - 1.0, float(np.float32(2.002)) - 2.0
    for k, length in enumerate(mr.THIN_LENGTHS):
        rows = np.arange(len(o)) % 4 == k
        assert (np.linalg.norm(d[rows], axis=1) == length).all()
        # the first pair is 0.0005 apart: skipped at every length, so medium 1 lasts from z = 1 to z = 2 and the boundary at 2 switches to 2
        skipped2 = gap2 / length < 0.001 - 1e-4
        on = abs(gap2 / length - 0.001) < 1e-4
        assert (ref.aside[rows].all() if on else ref.aside[rows].mean() < 0.02), length
        if on:
            continue
        tau = s1 * 1.0 + (0.0 if skipped2 else s2 * gap2)  # skipped: medium 2 lasts to the emitter at z = 3, whose own segment carries no factor (lib.rs:447-451)
        keep = rows & ~ref.aside
        assert (ref.tr[keep] == 0).all()  # tr meets the emitter's Matte wall
        np.testing.assert_allclose(mr.walk_reference("thin", 0, True).tr[keep], np.tile(np.exp(-tau) * np.float64(mr._L), (keep.sum(), 1)), rtol=1e-9)
        assert (ref.queries[keep] == (3 if skipped2 else 4)).all()
    assert {k for k, length in enumerate(mr.THIN_LENGTHS) if abs(gap2 / length - 0.001) < 1e-4} == {2} and gap1 / min(mr.THIN_LENGTHS) < 0.0009


def test_shell_and_ellipsoid_chords_in_closed_form():
    D = mr.walk_description("shells")
    ref = mr.walk_reference("shells", 3, False)  # from the centre: 0.3 of medium 3, 0.3 of medium 2, 0.4 of medium 1, whatever |rd|
    tau = 0.3 * _sigma(D, 3) + 0.3 * _sigma(D, 2) + 0.4 * _sigma(D, 1)
    free = ref.ended == 0
    np.testing.assert_allclose(ref.tr[free], np.tile(np.exp(-tau), (free.sum(), 1)), rtol=1e-6)  # the radii are fp32 numbers
    assert (ref.queries == 4).all() and (ref.tr[~free] == 0).all()
    # from outside: a chord of a sphere of radius r at distance b from the centre is 2 sqrt(r^2 - b^2)
    o, d = (v.astype(np.float64) for v in mr.walk_rays("shells", 0))
    ref = mr.walk_reference("shells", 0, False)
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    oc = o - np.float64(mr._CENTRE)
    b2 = (oc * oc).sum(-1) - (oc * u).sum(-1) ** 2
    chord = lambda r: 2 * np.sqrt(np.fmax(r * r - b2, 0.0))
    c1, c2, c3 = chord(1.0), chord(float(np.float32(0.6))), chord(float(np.float32(0.3)))
    tau = (c1 - c2)[:, None] * _sigma(D, 1) + (c2 - c3)[:, None] * _sigma(D, 2) + c3[:, None] * _sigma(D, 3)
    keep = (ref.ended == 0) & ~ref.aside
    assert keep.sum() > 300
    np.testing.assert_allclose(ref.tr[keep], np.exp(-tau)[keep], rtol=1e-5)
    assert (ref.queries[keep] == 3 + 2 * (c2[keep] > 0) + 2 * (c3[keep] > 0)).all()
    # the ellipsoid from its centre: the semi-axis along u is 1 / |(u.x, u.y / 0.5, u.z / 2)|
    D = mr.walk_description("ellipsoid")
    o, d = (v.astype(np.float64) for v in mr.walk_rays("ellipsoid", 1))
    ref = mr.walk_reference("ellipsoid", 1, False)
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    reach = 1.0 / np.linalg.norm(u / np.float64([1.0, 0.5, 2.0]), axis=1)
    free = ref.ended == 0
    np.testing.assert_allclose(ref.tr[free], np.exp(-reach[:, None] * _sigma(D, 1))[free], rtol=1e-9)
    assert (ref.queries == 2).all() and 0.5 <= reach.min() < 0.55 and 1.8 < reach.max() <= 2.0


@pytest.mark.parametrize("scene,start", mr.WALK_CASES)
def test_the_walk_rays_stay_within_the_cap_and_the_oracle_within_the_allowance(scene, start, oracle_mod):
    from rene_amd import api
    s = mr.walk_scene(scene)
    assert api.pack_info(s).features & (64 | 128) == 64 | 128  # FEAT_SMALL | FEAT_VOLPATH: flags 0 runs the item loop, FLAG_FORCE_BVH the tree
    o = oracle_mod.Oracle(s)
    ro, rd = mr.walk_rays(scene, start)
    out = {}
    for emit in (False, True):
        share, rows = mr.walk_aside_share(scene, start, emit)
        assert share <= mr.SET_ASIDE_CAP, (scene, start, emit, share, rows[:8])
        got = out[emit] = o.transmittance(emit, start, ro, rd)
        worst, bad, count = mr.walk_check(got, scene, start, emit)
        print(f"{scene} from medium {start}, emit {int(emit)}: set aside {100 * share:.1f} %, oracle error / allowance {worst:.3f}")
        assert not bad.any(), (scene, start, emit, np.nonzero(bad)[0][:8], got[bad][:3])
        assert not count.any(), (scene, start, emit, np.nonzero(count)[0][:8], got[count][:3])
    ref = mr.walk_reference(scene, start, True)
    _emit_forms_agree(out[False], out[True], ref)
    with pytest.raises(ValueError):
        o.transmittance(False, len(mr.walk_description(scene).media), ro[:2], rd[:2])


def _emit_forms_agree(tr, tr_emit, ref):
    """lib.rs:391-394 against 445-453: on a ray that meets no area light the two forms trace the same queries; a Matte wall ends both at 0,
    a miss ends tr at its product and tr_emit at 0."""
    keep = ~ref.aside
    blocked, miss = keep & (ref.ended == 1), keep & (ref.ended == 0)
    assert (tr[blocked, :3] == 0).all() and (tr_emit[blocked, :3] == 0).all() and (tr_emit[miss, :3] == 0).all()
    assert (tr[blocked | miss, 3] == tr_emit[blocked | miss, 3]).all()
    assert not miss.any() or (tr[miss, :3] > 0).all()

