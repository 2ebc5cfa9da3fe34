"""tests/light_reference.py against what the CPU offers, with no GPU: the oracle (an fp32 evaluation of the same specification, so the
reference's allowances apply to it), the restatement of the frame-wide stream in tests/test_gpu_frame_stream.py, closed forms, and the
reference's own aside shares on every case tests/test_gpu_light_fp64.py runs (the cap is a condition on the inputs)."""
import numpy as np
import pytest

import bsdf_reference as br
import gbuffer_reference as gr
import light_reference as lr
import transform_cases as tc
from rene_amd import abi, api
from test_gpu_frame_stream import TABLE_CASES, restate_frame
from test_gpu_parity import t1_check

U = 2.0 ** -24


# ---- the emit-object table and the point ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lr.POINT_CASES)
def test_emit_objects_are_the_packers(case):
    s = lr.scene(case)
    objects = lr.emit_objects(s)
    assert len(objects) == api.pack_info(s).emit_object_len > 0
    assert [e.instance for e in objects] == sorted(e.instance for e in objects)


@pytest.mark.parametrize("name", list(TABLE_CASES))
def test_emitter_point_against_the_restated_frame_stream(name):
    """Depth 0 of the frame-wide stream is the coin, then what rene_emit_sample draws: the object, the triangle, r and s.  512 frame seeds per
    case of test_gpu_frame_stream.py; the points within 6 u of the terms' magnitudes (its bound: two evaluations, each within gamma_3)."""
    scene, emitters = TABLE_CASES[name]()
    objects = lr.emit_objects(scene)
    assert len(objects) == len(emitters)
    if not emitters:
        return
    seeds = np.random.default_rng(3).integers(0, 2 ** 32, 512, dtype=np.uint64)
    rng = br.Rng(seeds, skip=1)  # behind the coin
    everyone = np.arange(len(seeds))
    obj = (rng.u32(everyone) % np.uint64(len(objects))).astype(np.int64)
    got = lr.emitter_point(objects, obj, rng)
    lights = 0
    for i, seed in enumerate(seeds):
        coin, _, on, scale = restate_frame(int(seed), emitters)
        if coin[0]:
            lights += 1
            assert (np.abs(got["point"][i] - on[0].astype(np.float64)) <= 6.000001 * U * scale[0]).all(), (name, i)
            assert got["draws"][i] == 3
    assert lights > 200


@pytest.mark.parametrize("case", lr.POINT_CASES)
def test_every_point_lies_on_its_emitter(case):
    objects = lr.emit_objects(lr.scene(case))
    seeds = np.concatenate([np.random.default_rng(4).integers(0, 2 ** 32, lr.N_SEEDS, dtype=np.uint64), [s for s, _, _ in lr.SUM_SEEDS.values()]])
    ref = lr.emit_sample(objects, seeds)
    assert ref["aside"].mean() <= lr.EDGE_CAP and np.isfinite(ref["point"]).all() and (ref["allow"] >= 0).all()
    for k, e in enumerate(objects):
        w = np.nonzero(ref["obj"] == k)[0]
        assert len(w) > 0
        if e.sphere:
            if abs(np.linalg.det(e.matrix[:3, :3])) > 0:
                p = (ref["point"][w] - e.matrix[:3, 3]) @ np.linalg.inv(e.matrix[:3, :3]).T
                assert np.abs(np.linalg.norm(p, axis=1) - 1.0).max() < 1e-12
            assert (ref["draws"][w] == 3 * ref["rounds"][w]).all() and ref["rounds"][w].min() >= 1
        else:
            r, s = ref["r"][w], ref["s"][w]
            # 1 + 2^-24 is no fp32 number: the sum rounds to 1, the fold is not taken and b0 = -2^-24 (light_reference.SUM_SEEDS, "above")
            assert (r >= 0).all() and (s >= 0).all() and (r <= 1).all() and (s <= 1).all() and (1.0 - r - s >= -U).all()
            assert (ref["prim"][w] >= 0).all() and (ref["prim"][w] < e.prim_count).all() and (ref["draws"][w] == 3).all()
            ts = e.triangles
            off = ((ref["point"][w] - e.vertices[e.indices[ref["prim"][w], 0]]) * ts.unit_n[ref["prim"][w]]).sum(1)
            assert np.abs(off).max() < 1e-12  # in its triangle's plane


def test_the_crafted_sums():
    """SUM_SEEDS: the third and fourth draws sum to 2^24 - 1, 2^24, 2^24 + 1, 2^24 + 2 over 2^24; only the last folds."""
    for name, total, fold in (("below", -1, False), ("one", 0, False), ("above", 1, False), ("fold", 2, True)):
        seed, r, s = lr.SUM_SEEDS[name]
        draws = [int(v) for v in br._output(np.array([br._step(br._step(br.pcg_new(seed)))[0], br._step(br._step(br._step(br.pcg_new(seed))))[0]], np.uint64))]
        assert [d >> 8 for d in draws] == [r, s] and r + s == (1 << 24) + total
        assert bool(np.float32(r * U) + np.float32(s * U) > np.float32(1.0)) == fold
    for k, t in ((0, 0xFFFFFFF0), (1, 5), (2, 77), (3, 123456)):
        seed, target = lr.seed_with_draw(k, range(t, t + 64))
        rng = br.Rng(np.array([seed], np.uint64), skip=k)
        assert int(rng.u32(np.arange(1))[0]) == target


# ---- the pdf ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lr.PDF_CASES)
def test_emitter_pdf_against_the_oracle(case, oracle_mod):
    """The oracle's fp64 column (the sphere formula) to the rounding of pi, and its fp32 pdf inside the allowance on every ray."""
    o, d = lr.pdf_rays(case)
    objects, hit = lr.pdf_reference(case)
    f32, f64 = oracle_mod.Oracle(lr.scene(case)).emitter_pdf(o, d)
    pdf, allow, aside = lr.emitter_pdf(objects, hit, o, d)
    both = ~aside & (f64 > 0) & np.isfinite(pdf) & (pdf > 0)
    if both.any():  # (the reference multiplies by the specification's fp32 pi, the oracle's double by pi)
        assert (np.abs(pdf[both] - f64[both]) <= (U + 1e-12) * f64[both]).all()
    ok, ratio, aside = lr.pdf_check(f32, objects, hit, o, d)
    print(f"{case}: {len(o)} rays, the oracle's fp32 pdf at most {ratio:.3f} of the allowance, asides {aside.mean():.4f}")
    assert ok.all(), (case, int((~ok).sum()), np.nonzero(~ok)[0][:4])
    assert np.array_equal(f32[~aside] > 0, hit["t"][~aside] > 0)


def _solid_angle(corners, p):
    """Van Oosterom and Strackee: the solid angle of the triangle `corners` (3, 3) seen from p."""
    a, b, c = (corners - p)
    la, lb, lc = np.linalg.norm(a), np.linalg.norm(b), np.linalg.norm(c)
    return abs(2.0 * np.arctan2(np.dot(a, np.cross(b, c)), la * lb * lc + np.dot(a, b) * lc + np.dot(a, c) * lb + np.dot(b, c) * la))


def test_one_over_pdf_integrates_to_the_solid_angle():
    """An unoccluded sphere: the cone's 1 / pdf IS its solid angle.  A quad of two triangles: the mean of 1 / pdf over the sampler's own points
    (which have that pdf) estimates the quad's solid angle, compared with Van Oosterom and Strackee's within 5 standard errors."""
    s = lr.scene("veach")
    objects = lr.emit_objects(s)
    e = objects[0]
    origin = np.array([[3.0, 2.0, 1.0]], np.float32)
    d = (e.matrix[:3, 3] - origin).astype(np.float32)
    hit = lr.Tracer(s, 1).trace(origin, d)
    pdf, _, _ = lr.emitter_pdf(objects, hit, origin, d)
    radius, dist = tc.quirk_radius(e.matrix.astype(np.float32)), np.linalg.norm(e.matrix[:3, 3] - origin[0])
    assert hit["instance"][0] == e.instance and abs(1.0 / pdf[0] - lr.solid_angle_of_sphere(radius, dist)) < 2 * U / pdf[0]
    s = lr.scene("cornell")
    objects = lr.emit_objects(s)
    n = 20000
    ref = lr.emit_sample(objects, np.arange(n))
    p = np.array([0.3, 0.7, -0.2])
    d = ref["point"] - p
    hit = lr.Tracer(s, 1).trace(np.broadcast_to(p, d.shape).copy(), d)
    pdf, _, aside = lr.emitter_pdf(objects, hit, np.broadcast_to(p, d.shape).copy(), d)
    assert (hit["t"] > 0).mean() > 0.999 and aside.mean() < lr.EDGE_CAP
    est = np.where(pdf > 0, 1.0 / np.maximum(pdf, 1e-300), 0.0)
    want = sum(_solid_angle(objects[0].vertices[t], p) for t in objects[0].indices)
    assert abs(est.mean() - want) <= 5.0 * est.std() / np.sqrt(n), (est.mean(), want)


def test_lambert_closed_form_is_the_bsdf_references():
    """_lambert against bsdf_reference.evaluate on the shared scene's Matte: f(wo, wi), and the integrator's pdf(wi, normal) (Q1)."""
    sh = br.shared_scene()
    rng = np.random.default_rng(7)
    n = 512
    unit = lambda: (lambda v: (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32))(rng.normal(size=(n, 3)))
    nrm, wo, wi = unit(), unit(), unit()
    mat = next(i for i, m in enumerate(sh.scene.materials) if m.type == abi.MATERIAL_MATTE and sh.scene.textures[m.u0[0]].type == abi.TEXTURE_SOLID)
    R = np.asarray(sh.scene.textures[sh.scene.materials[mat].u0[0]].v0[:3], np.float64)
    uv = np.zeros((n, 2), np.float32)
    f, pdf, _, _ = lr._lambert(R, lr._unit(nrm.astype(np.float64)), wo.astype(np.float64), wi.astype(np.float64))
    e = br.evaluate(sh.scene, mat, nrm, uv, wo, wi)
    q1 = br.evaluate(sh.scene, mat, nrm, uv, wi, nrm)
    keep = ~e.aside["f"] & ~q1.aside["pdf"]
    assert keep.mean() > 0.9
    assert (np.abs(f - e.f)[keep] <= e.f_allow[keep] + 1e-12).all() and (np.abs(pdf - q1.pdf)[keep] <= q1.pdf_allow[keep] + 1e-12).all()


# ---- the direct-light pass ----------------------------------------------------------------------------------------------------------------------------
_direct = {}


def _direct_reference(case, oracle_mod):
    """direct_sample on the oracle's primary hits and the BSDF reference's wi: (reference, frames, W, H), once per process."""
    if case not in _direct:
        s, n = lr.scene(case), lr.DIRECT_CASES[case]
        W, H = s.film.xresolution, s.film.yresolution
        ph = gr.reference_samples(oracle_mod, oracle_mod.Oracle(s), W, H, 0, n, edges=False)["samples"].reshape(-1)
        seeds = lr.direct_inputs(case, n)
        _direct[case] = (lr.direct_sample(s, seeds, ph, lr.reference_wi(s, seeds, ph, W, H)), n, W, H)
    return _direct[case]


def test_direct_sums_against_the_capped_renders(oracle_mod):
    """Cornell 48 x 40 x 8 frames: seen + distant is the oracle's depth_cap = 1 render and seen + distant + sampled its depth_cap = 2 render,
    under t1_check's defaults -- the reference held to the oracle before it judges a device."""
    ref, n, W, H = _direct_reference("cornell", oracle_mod)
    assert (W, H, n) == (48, 40, 8)
    first, both = np.zeros((n * H * W, 3)), np.zeros((n * H * W, 3))
    first[ref["rows"]] = ref["seen"] + ref["distant"]
    both[ref["rows"]] = ref["seen"] + ref["distant"] + ref["sampled"]
    for cap, img in ((1, first), (2, both)):
        o = oracle_mod.Oracle(lr.scene("cornell"))
        o.set_experiment(depth_cap=cap)
        o.render(0, n)
        want = o.download(0)
        got = img.reshape(n, H, W, 3).sum(0).astype(np.float32)
        print(f"cap {cap}: relMSE {float(((got - want) ** 2).sum() / max(1e-30, float((want ** 2).sum()))):.3g}")
        t1_check(got, want)
    assert both.sum() > first.sum() > 0


# ---- the aside shares of the GPU cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lr.PDF_CASES)
def test_aside_share_of_the_pdf_cases(case):
    _, hit = lr.pdf_reference(case)
    print(f"{case}: asides {hit['aside'].mean():.4f}")
    assert hit["aside"].mean() <= lr.EDGE_CAP


@pytest.mark.parametrize("case", list(lr.DIRECT_CASES))
def test_aside_share_and_coverage_of_the_direct_cases(case, oracle_mod):
    """From the reference alone (the oracle's primary hits, the BSDF reference's wi): asides at most 0.5 % outside the exemption, at least 50
    judged samples on each side of the coin, at least 20 whose wi grazes the emitter it hits (|cos| < 0.05)."""
    ref, n, W, H = _direct_reference(case, oracle_mod)
    share = float((ref["aside"] & ~ref["exempt"]).mean())
    cos = lr.emitter_cosine(lr.scene(case), ref)
    with np.errstate(invalid="ignore"):
        grazing = int(((cos < 0.05) & ~ref["aside"]).sum())
    print(f"{case}: {len(ref['rows'])} samples, asides {share:.4f}, exempt {ref['exempt'].mean():.4f}, light {int(ref['light'].sum())}, "
          f"bsdf {int((~ref['light']).sum())}, grazing the emitter {grazing}")
    assert share <= lr.EDGE_CAP
    assert (ref["light"] & ~ref["aside"]).sum() >= 50 and (~ref["light"] & ~ref["aside"]).sum() >= 50 and grazing >= 20
