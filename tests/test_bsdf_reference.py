"""CPU: the fp64 BSDF reference of tests/bsdf_reference.py against closed forms it was not written from; the oracle within the reference's
allowance on the inputs the GPU test uses (lobe counts exact); and the set-aside caps, which are conditions on the inputs that the reference
alone has to meet.  The oracle's probe reports how many random numbers its sample drew: the count is the reference's wherever no decision of the sample
is in doubt."""
import json
import math
import os

import numpy as np
import pytest

import bsdf_reference as br
from conftest import GOLDEN

S = br.shared_scene()
Z = np.float64([[0.0, 0.0, 1.0]])


def _dir(theta, phi):
    return np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta) * np.ones_like(phi)], -1)


def _tile(v, n):
    return np.tile(np.float64(v), (n, 1))


# ---- the generator -----------------------------------------------------------------------------------------------------------------------------------------
def test_pcg32si_restatement_meets_the_known_answers():
    with open(os.path.join(GOLDEN, "pcg32si_kat.json")) as f:
        kat = json.load(f)
    one = np.array([0])
    for seed, want in kat.items():
        r = br.Rng([int(seed)])
        assert int(r.state[0]) == want["state_after_new"]
        assert [int(r.u32(one)[0]) for _ in range(8)] == want["u32"]
        r = br.Rng([int(seed)])
        assert [float(r.f32(one)[0]) for _ in range(8)] == [v * 2.0 ** -24 for v in want["f32_bits_num"]]
    assert int(r.draws[0]) == 8


def test_edge_seeds_draw_what_their_rows_say():
    rows, one = br.edge_rows(), np.array([0])

    def draws(name):
        r = br.Rng([rows[name][3]])
        return int(r.u32(one)[0]), int(r.u32(one)[0])
    assert draws("first draw below 2^8")[0] < 2 ** 8
    assert draws("first draw 2^31")[0] >= 2 ** 31
    assert draws("first draw 0xFFFFFFxx")[0] >> 8 == 0xFFFFFF
    assert draws("first next_f32 is 0")[1] >> 8 == 0                     # the first draw picks the lobe: the second is the first next_f32
    assert (draws("first next_f32 is 1 - 2^-24")[1] >> 8) * 2.0 ** -24 == 1.0 - 2.0 ** -24


def test_edge_rows_are_normal_floats():
    I = br.edge_set()
    for v in (I.n, I.wo, I.wi):
        assert np.isfinite(v).all() and ((v == 0) | (np.abs(v) >= 2.0 ** -60)).all()
    # with n = +z the frame is u = +y, v = -x: the local directions are the rows' own numbers
    u, v, w = br.onb_from_w(Z)
    assert np.array_equal(u, [[0, 1, 0]]) and np.array_equal(v, [[-1, 0, 0]]) and np.array_equal(w, Z)
    u, v, w = br.onb_from_w(br._unit(np.float64([[0.5, -0.5, 0.7071068]])))  # a tie takes the second form (math.rs:90-94)
    assert u[0, 0] == 0 and abs(br._dot(u, v)[0]) < 1e-15 and abs(br._dot(v, w)[0]) < 1e-15


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------------------------
def test_lambert_is_albedo_over_pi_and_cosine_over_pi():
    n = 64
    rng = np.random.default_rng(1)
    wo, wi = _dir(rng.uniform(0, 1.5, n), rng.uniform(0, 6.28, n)), _dir(rng.uniform(0, 1.5, n), rng.uniform(0, 6.28, n))
    e = br.evaluate(S.scene, S.material["matte"], _tile(Z[0], n), np.zeros((n, 2)), wo, wi)
    np.testing.assert_allclose(e.f, _tile(np.float32([0.6, 0.4, 0.2]).astype(np.float64) / math.pi, n), rtol=1e-7)  # fp32(1 / pi) is 1 / pi to 3e-8
    np.testing.assert_allclose(e.pdf, wi[:, 2] / math.pi, rtol=1e-7)
    e = br.evaluate(S.scene, S.material["matte"], _tile(Z[0], n), np.zeros((n, 2)), wo, wi * [1, 1, -1])
    assert (e.f == 0).all() and (e.pdf == 0).all()  # across the surface: no transmission lobe, and not the same hemisphere


def test_dielectric_fresnel_closed_forms():
    for ir in (1.5, 1.33, 1.0001):
        r0 = ((ir - 1) / (ir + 1)) ** 2
        assert br.fr_dielectric(1.0, 1.0, ir) == pytest.approx(r0, rel=1e-12)
        assert br.fr_dielectric(-1.0, 1.0, ir) == pytest.approx(r0, rel=1e-12)              # from inside: the indices swap
        brewster = math.cos(math.atan(ir))                                                    # r_parl == 0: F = r_perp^2 / 2, r_perp = (1 - n^2) / (1 + n^2)
        assert br.fr_dielectric(brewster, 1.0, ir) == pytest.approx(0.5 * ((1 - ir * ir) / (1 + ir * ir)) ** 2, rel=1e-9)
        critical = math.sqrt(1 - 1 / (ir * ir))
        assert br.fr_dielectric(-critical * 0.999, 1.0, ir) == 1.0                            # past the critical angle
        assert br.fr_dielectric(-critical * 1.001, 1.0, ir) < 1.0
        assert br.fr_dielectric(critical * 0.5, 1.0, ir) < 1.0                                # no total reflection from outside
    assert br.fr_dielectric(0.0, 1.0, 1.5) == pytest.approx(1.0, abs=1e-12)


def test_conductor_fresnel_at_normal_incidence():
    eta, k = np.float64([br.ETA]), np.float64([br.K])
    want = ((eta - 1) ** 2 + k ** 2) / ((eta + 1) ** 2 + k ** 2)  # |(n - 1) / (n + 1)|^2, n = eta + i k
    np.testing.assert_allclose(br.fr_conductor(np.float64([1.0]), eta, k), want, rtol=1e-12)


@pytest.mark.parametrize("ax,ay", [(0.25, 0.25), (0.1, 0.3)])
def test_d_times_cosine_integrates_to_one(ax, ay):
    nt, nphi = 4000, 512
    th, ph = (np.arange(nt) + 0.5) / nt * (math.pi / 2), (np.arange(nphi) + 0.5) / nphi * (2 * math.pi)
    t, p = (a.reshape(-1) for a in np.meshgrid(th, ph, indexing="ij"))
    d = br.tr_d(np.float64(ax), np.float64(ay), _dir(t, p))
    total = (d * np.cos(t) * np.sin(t)).sum() * (math.pi / 2 / nt) * (2 * math.pi / nphi)
    assert total == pytest.approx(1.0, rel=1e-5)  # pi as fp32 is in D: 3e-8


@pytest.mark.parametrize("case", ["metal-0.1", "metal-aniso", "metal-image", "substrate", "substrate-aniso", "plastic-nokd"])
def test_f_is_reciprocal(case):
    n = 256
    rng = np.random.default_rng(5)
    wo, wi = _dir(rng.uniform(0.05, 1.5, n), rng.uniform(0, 6.28, n)), _dir(rng.uniform(0.05, 1.5, n), rng.uniform(0, 6.28, n))
    uv = rng.uniform(0, 1, (n, 2))
    a = br.evaluate(S.scene, S.material[case], _tile(Z[0], n), uv, wo, wi)
    b = br.evaluate(S.scene, S.material[case], _tile(Z[0], n), uv, wi, wo)
    assert (a.f > 0).all()
    np.testing.assert_allclose(a.f, b.f, rtol=1e-9)


@pytest.mark.parametrize("case,ir", [("glass-1.5", 1.5), ("glass-1.0001", 1.0001)])
def test_the_refracted_direction_obeys_snell(case, ir):
    n, ir = 512, float(np.float32(ir))  # the material holds the index in fp32
    rng = np.random.default_rng(6)
    wo = _dir(rng.uniform(0.0, math.pi, n), rng.uniform(0, 6.28, n))
    s = br.sample(S.scene, S.material[case], _tile(Z[0], n), np.zeros((n, 2)), wo, rng.integers(0, 1 << 32, n, dtype=np.uint64))
    refracted = (s.dec.items["s0.coin<F"][1] == 0) & (s.pdf > 0)
    assert refracted.sum() > n // 4
    sin_o, sin_i = np.hypot(wo[:, 0], wo[:, 1])[refracted], np.hypot(s.wi[:, 0], s.wi[:, 1])[refracted]
    outside = wo[refracted, 2] > 0
    np.testing.assert_allclose(np.where(outside, sin_o, ir * sin_o), np.where(outside, ir * sin_i, sin_i), rtol=1e-9, atol=1e-12)
    assert (np.sign(s.wi[refracted, 2]) == -np.sign(wo[refracted, 2])).all()
    np.testing.assert_allclose(np.linalg.norm(s.wi[refracted], axis=1), 1.0, rtol=1e-9)
    mirrored = s.dec.items["s0.coin<F"][1] == 1
    np.testing.assert_allclose(s.wi[mirrored], (wo * [-1, -1, 1])[mirrored], atol=1e-15)  # with n = +z the local mirror (-x, -y, z) is the world's


@pytest.mark.parametrize("case", br.SINGLE_NON_SPECULAR)
def test_a_sample_carries_the_f_and_pdf_of_its_own_direction(case):
    I = br.uniform_set(case)
    _, sm = br.reference(case, "uniform")
    ev = br.evaluate(S.scene, S.material[case], I.n, I.uv, I.wo, sm.wi)  # the sampled wi handed over in float64
    drawn = sm.pdf > 0
    assert drawn.mean() > 0.3
    np.testing.assert_allclose(ev.pdf[drawn], sm.pdf[drawn], rtol=1e-6)
    np.testing.assert_allclose(ev.f[drawn], sm.f[drawn], rtol=1e-6, atol=1e-300)


@pytest.mark.parametrize("case", br.CASES)
def test_lobe_counts(case):
    """material.rs:579-630, 680-707: a lobe per colour that is not zero; the table in bsdf_reference.LOBE_COUNTS is stated by hand."""
    for which in br.SETS:
        ev, sm = br.reference(case, which)
        assert (ev.len == br.LOBE_COUNTS[case]).all() and (sm.len == br.LOBE_COUNTS[case]).all()
        assert (sm.lobe < np.maximum(sm.len, 1)).all() and ((sm.lobe >= 0) == (sm.len > 0)).all()
    if br.LOBE_COUNTS[case] > 1:
        assert set(np.unique(br.reference(case, "uniform")[1].lobe)) == set(range(br.LOBE_COUNTS[case]))  # every lobe is drawn


def test_a_real_defect_is_far_outside_the_allowance():
    """For scale: Plastic's Fresnel with its indices the other way round, and a pdf without the abs, against the allowance of the same samples."""
    ev, _ = br.reference("plastic-nokd", "uniform")
    I = br.uniform_set("plastic-nokd")
    L = br.lobes(S.scene, S.material["plastic-nokd"], I.uv)
    L[1]["eta_i"], L[1]["eta_t"] = 1.0, 1.5  # lobe 0 is the Lambert lobe that kd = 0 leaves out
    onb = br._frame(I.n)
    wo, wi = br._to_local(onb, br._in(I.wo)), br._to_local(onb, br._in(I.wi))
    f, _, _, _ = br._evaluate(L, wo, wi, br.Moves(np.zeros((len(wo), 3))))
    lit = (ev.f[:, 0] > 1e-3) & ~ev.aside["f"]
    assert lit.sum() > 100
    assert np.median((np.abs(f - ev.f)[lit] / ev.f_allow[lit])) > 1e3


# ---- the caps and the oracle -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", br.CASES)
def test_the_inputs_stay_within_the_set_aside_caps(case):
    for which in br.SETS:
        shares = br.aside_shares(case, which)
        print(f"{case} {which}: set aside " + ", ".join(f"{q} {100 * s:.1f} %" for q, (s, _) in shares.items()))
        cap = 0.0 if which == "edge" else br.SET_ASIDE_CAP
        for q, (share, rows) in shares.items():
            assert share <= cap, (case, which, q, share, [br.edge_set().names[i] for i in rows] if which == "edge" else rows[:8])


def test_every_exemption_names_rows_of_the_edge_set():
    names = br.edge_set().names
    for prefix, (quantities, cases, reason) in br.EDGE_EXEMPT.items():
        assert any(k.startswith(prefix) for k in names) and set(quantities) <= set(br.QUANTITIES) and reason
        assert cases is None or set(cases) <= set(br.CASES)


@pytest.mark.parametrize("case", br.CASES)
def test_the_oracle_stays_within_the_allowance(case, oracle_mod):
    for which in br.SETS:
        rows = br.oracle_rows(oracle_mod, case, which)
        result, counts = br.check(rows, case, which)
        _, sm = br.reference(case, which)
        same = rows[:, 12] == sm.draws  # the stream is consumed identically wherever no decision of the sample is in doubt
        assert same[~sm.flipped].all(), (case, which, "draws", np.nonzero(~same & ~sm.flipped)[0][:8], rows[:, 12][~same][:8], sm.draws[~same][:8])
        print(f"{case} {which}: oracle error / allowance " + ", ".join(f"{q} {r:.2f}" for q, (r, _) in result.items()))
        assert counts, (case, which)
        for q, (_, bad) in result.items():
            assert not bad.any(), (case, which, q, int(bad.sum()), np.nonzero(bad)[0][:8], rows[bad][:3])
