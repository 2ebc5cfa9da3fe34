"""-m gpu: the light side of the render path -- the point sampled on an emitter (rene_emit_sample), the emitter pdf (rene_emitter_pdf_form), and
the direct-light pass's samples on Lambert surfaces (rene_direct_samples) -- against the float64 reference of tests/light_reference.py, per
sample, within its counted, conditioning-scaled allowances.  Flags 0 and FLAG_FORCE_BVH; on a small-scene context every probe form: 0 the
global tables (emit_sample, emitter_pdf), 1 and 2 the LDS image (emit_sample_lds, emitter_pdf_lds<.., false / true>) that the small-scene render
kernels read.  An aside (light_reference: a decision within its budget of flipping) is held to the union of the admissible answers; the share
of asides per case is capped from the reference alone in tests/test_light_reference.py.  Each test prints the largest |device - reference| /
allowance it met; DESIGN.md (oracle status) records them.

Two one-line changes of device_code.inc on a scratch build, each of which a whole render's tolerances absorb, fail these tests: `q[16]` read
as `q[15]` in emitter_pdf_lds (the area where primitive_count stands) fails test_emitter_pdf on every small scene with a triangle emitter
(cornell, many-emitters, mixed and the three quads: forms 1 and 2), and r and s swapped in emit_sample_lds fails test_emitter_points on the
same six (the point, and forms 0 and 1 no longer bit for bit equal); the sphere-only and the BVH scenes, which do not run the changed
lines, pass."""
import numpy as np
import pytest

import light_reference as lr
from rene_amd import abi, api

pytestmark = pytest.mark.gpu

FLAGS = (0, abi.FLAG_FORCE_BVH)


def _contexts(case):
    """(flags, renderer, the probe forms the context admits) for both flag settings; asserts which forms a context must admit."""
    s = lr.scene(case)
    small = bool(api.pack_info(s).features & abi.FEAT_SMALL)
    for flags in FLAGS:
        with api.Renderer(s, flags=flags) as r:
            lds = small and not flags
            for form in (1, 2):  # the LDS forms exist exactly on the contexts whose render kernels read the image
                if not lds:
                    with pytest.raises(api.ReneError) as e:
                        r.emitter_pdf_form(form, np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32))
                    assert e.value.code == -1
            if not lds:
                with pytest.raises(api.ReneError) as e:
                    r.emit_sample(1, np.zeros(1, np.uint32))
                assert e.value.code == -1
            yield flags, r, lds


# ---- emitter points -----------------------------------------------------------------------------------------------------------------------------------
def _crafted_seeds(objects):
    """Seeds whose draws sit on the sampler's edges (light_reference.seed_with_draw inverts the generator): draw 0 picks the object, and for a
    triangle object draw 1 the triangle, draws 2 and 3 r and s."""
    seeds = []
    n_obj, top = len(objects), 0xFFFFFFFF
    for k in (0, 1):  # a u32 of 0xFFFFFFFF (the nearest below it that has a seed: only every other state has one) as the object's and as the primitive's draw
        seeds.append(lr.seed_with_draw(k, range(top, top - 64, -1))[0])
    seeds.append(lr.seed_with_draw(0, range(n_obj - 1, 1 << 32, n_obj))[0])  # u32 % emit_object_len on its last value, from the smallest u32 up
    for e in objects:
        if not e.sphere:
            seeds.append(lr.seed_with_draw(1, [e.prim_count - 1])[0] if lr.seed_for_draw(1, e.prim_count - 1) is not None else
                         lr.seed_with_draw(1, range(e.prim_count - 1, 1 << 32, e.prim_count))[0])
    seeds.append(lr.seed_with_draw(2, range(256))[0])  # r = 0
    seeds.append(lr.seed_with_draw(3, range(256))[0])  # s = 0
    seeds += [s for s, _, _ in lr.SUM_SEEDS.values()]  # r + s at 1 - 2^-24, 1, 1 + 2^-24 (which fp32 rounds to 1: no fold, b0 = -2^-24) and 1 + 2^-23
    return np.asarray(seeds, np.uint32)


@pytest.mark.parametrize("case", lr.POINT_CASES)
def test_emitter_points(case):
    """4096 random seeds, the crafted ones, and the 32 seeds of the first 65536 whose rejection loop runs longest: the point within its
    allowance, the object and the stream's next u32 equal (the device draws exactly the reference's count), forms 0 and 1 bit for bit equal."""
    objects = lr.emit_objects(lr.scene(case))
    assert len(objects) == api.pack_info(lr.scene(case)).emit_object_len > 0
    rng = np.random.default_rng(sum(map(ord, case)) + 1)
    seeds = np.concatenate([rng.integers(0, 2 ** 32, lr.N_SEEDS, dtype=np.uint64).astype(np.uint32), _crafted_seeds(objects)])
    if any(e.sphere for e in objects):
        first = lr.emit_sample(objects, np.arange(1 << 16))
        seeds = np.concatenate([seeds, np.argsort(-first["rounds"], kind="stable")[:32].astype(np.uint32)])
    ref = lr.emit_sample(objects, seeds)
    if any(e.sphere for e in objects):
        assert ref["rounds"].max() >= 6
    assert ref["aside"].mean() <= lr.EDGE_CAP
    forms_run = {}
    for flags, r, lds in _contexts(case):
        got = {form: r.emit_sample(form, seeds) for form in ((0, 1) if lds else (0,))}
        forms_run[flags] = tuple(got)
        if lds:
            assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)), (case, "forms 0 and 1 differ")
        for form, g in got.items():
            bits = g.view(np.uint32)
            assert not bits[:, 5:].any()
            keep = ~ref["aside"]  # (a rejection test within its budget of 1: either continuation is admissible; none among these seeds)
            assert np.array_equal(bits[keep, 3], ref["obj"][keep].astype(np.uint32)), (case, flags, form, "object")
            assert np.array_equal(bits[keep, 4], ref["next"][keep]), (case, flags, form, "the stream's position")
            err = np.abs(g[:, :3].astype(np.float64) - ref["point"])
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(err == 0, 0.0, err / ref["allow"])
            bad = keep & ~(ratio <= 1.0).all(1)
            worst = float(ratio[keep].max())
            print(f"{case}, flags {flags}, form {form}: {len(seeds)} seeds, largest |point - reference| / allowance {worst:.3f}, asides {ref['aside'].mean():.4f}")
            assert not bad.any(), (case, flags, form, int(bad.sum()), np.nonzero(bad)[0][:4], worst)
    small = bool(api.pack_info(lr.scene(case)).features & abi.FEAT_SMALL)
    assert forms_run == {0: (0, 1) if small else (0,), abi.FLAG_FORCE_BVH: (0,)}, forms_run


def test_emit_sample_refuses_a_scene_without_emitters():
    from test_gpu_frame_stream import no_emitters
    with api.Renderer(no_emitters()[0]) as r:
        for form in (0, 1):
            with pytest.raises(api.ReneError) as e:
                r.emit_sample(form, np.zeros(4, np.uint32))
            assert e.value.code == -1
        assert (r.emitter_pdf_form(1, np.zeros((3, 3), np.float32), np.ones((3, 3), np.float32)) == 0).all()  # no emitter: every ray misses


# ---- the emitter pdf ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lr.PDF_CASES)
def test_emitter_pdf(case):
    """The ray sets of test_gpu_probes.py and test_gpu_transforms.py with their grazing rays kept, rays within 1e-3 rad of a flat emitter's
    plane and origins at 2 to 200 radii from a sphere: every ray inside the scaled allowance, the same rays hit, +inf on exactly the
    reference's rays (`cyclic`); form 2 against form 1 within the allowance of one more normalize."""
    o, d = lr.pdf_rays(case)
    objects, hit = lr.pdf_reference(case)
    assert hit["aside"].mean() <= lr.EDGE_CAP
    forms_run = {}
    for flags, r, lds in _contexts(case):
        got = {form: r.emitter_pdf_form(form, o, d) for form in ((0, 1, 2) if lds else (0,))}
        forms_run[flags] = tuple(got)
        assert np.array_equal(got[0].view(np.uint32), r.emitter_pdf(o, d).view(np.uint32))  # form 0 is rene_emitter_pdf
        for form, g in got.items():
            ok, ratio, aside = lr.pdf_check(g, objects, hit, o, d, extra_normalise=form == 2)
            print(f"{case}, flags {flags}, form {form}: {len(o)} rays, {int((hit['t'] > 0).sum())} hits, largest |pdf - reference| / allowance {ratio:.3f}, "
                  f"asides {aside.mean():.4f}")
            bad = np.nonzero(~ok)[0]
            assert not len(bad), (case, flags, form, len(bad), bad[:4], g[bad[:4]], lr.emitter_pdf(objects, hit, o, d)[0][bad[:4]], ratio)
            keep = ~aside
            assert np.array_equal(g[keep] > 0, hit["t"][keep] > 0), (case, flags, form, "the same rays hit")
            if case == "ball/cyclic":
                assert np.array_equal(np.isposinf(g[keep]), hit["t"][keep] > 0) and (hit["t"] > 0).sum() > 3000
            else:
                assert np.isfinite(g).all()
        if lds:
            pdf, allow, aside = lr.emitter_pdf(objects, hit, o, d, extra_normalise=True)
            both = ~aside & (hit["t"] > 0) & np.isfinite(pdf)
            with np.errstate(invalid="ignore"):  # (inf - inf on `cyclic`, whose rays `both` leaves out)
                diff = np.abs(got[2].astype(np.float64) - got[1])[both]
            with np.errstate(invalid="ignore", divide="ignore"):
                rel_one = _one_normalise(objects, hit, o, d)[both]
            worst = float((diff / (rel_one * pdf[both])).max()) if both.any() else 0.0
            print(f"{case}: form 2 against form 1, largest difference {float((diff / pdf[both]).max()) if both.any() else 0.0:.3g} of the pdf, "
                  f"{worst:.3f} of one normalize's allowance")
            assert worst <= 1.0, (case, worst)
    small = bool(api.pack_info(lr.scene(case)).features & abi.FEAT_SMALL)
    assert forms_run == {0: (0, 1, 2) if small else (0,), abi.FLAG_FORCE_BVH: (0,)}, forms_run


def _one_normalise(objects, hit, o, d):
    """What form 2 may differ from form 1 by, relative to the pdf, per ray.  A sphere's pdf does not read the direction: the two rounded
    quotients each form ends on.  A triangle's: the cosine of a direction sqrt(3) N_NORMALISE u off, over the cosine; the hit point of a ray
    turned by that angle, twice over the cosine for d^2; and the traversal's own roundings, drawn afresh for the new direction, in both forms
    (the B_TRI_POS term of the allowance, twice).  What both forms share -- the packer's normal and area, the arithmetic behind the hit
    point -- is not in it."""
    rel = np.full(len(o), 8.0 * lr.U)
    dd = np.asarray(d, np.float64)
    oo = np.asarray(o, np.float64)
    for e in objects:
        w = np.nonzero((hit["t"] > 0) & (hit["instance"] == e.instance))[0]
        if e.sphere or not len(w):
            continue
        prim = hit["primitive"][w]
        dlen = np.linalg.norm(dd[w], axis=1)
        cos = np.abs((dd[w] * e.triangles.unit_n[prim]).sum(1)) / dlen
        size = np.maximum(np.linalg.norm(oo[w], axis=1), np.linalg.norm(e.vertices[e.indices[prim]], axis=2).max(1))
        turn = np.sqrt(3.0) * lr.N_NORMALISE
        rel[w] = lr.U * (8.0 + (3.0 * turn + 2.0 * lr.B_TRI_POS * e.triangles.thin[prim] * size / (hit["t"][w] * dlen)) / cos)
    return rel


# ---- direct samples on the Matte scenes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("case", list(lr.DIRECT_CASES))
def test_direct_samples(case, flags):
    """Every sample of rene_direct_samples whose primary hit is a Lambert surface, against light_reference.direct_sample fed with the device's own
    primary hits (rene_primary_hits) and, for the BSDF-state rows, the device's own wi: state, second, seen, wi (an angle), pdf, distant and
    sampled within the allowances; at least 50 judged samples on each side of the coin and 20 whose wi grazes the emitter it hits."""
    s, n = lr.scene(case), lr.DIRECT_CASES[case]
    with api.Renderer(s, flags=flags) as r:
        ph = r.primary_hits(0, n)
        smp = r.direct_samples(0, n)
    ref = lr.direct_sample(s, lr.direct_inputs(case, n), ph.reshape(-1), smp["wi"].reshape(-1, 3))
    passed, worst = lr.direct_check(smp, ref)
    share = float((ref["aside"] & ~ref["exempt"]).mean())
    cos = lr.emitter_cosine(s, ref)
    with np.errstate(invalid="ignore"):
        grazing = int(((cos < 0.05) & ~ref["aside"]).sum())
    light, bsdf = int((ref["light"] & ~ref["aside"]).sum()), int((~ref["light"] & ~ref["aside"]).sum())
    print(f"{case}, flags {flags}: {len(ref['rows'])} Lambert samples (light {light}, bsdf {bsdf}, grazing the emitter {grazing}), asides {share:.4f}, "
          f"exempt {ref['exempt'].mean():.4f}; largest |device - reference| / allowance: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    bad = np.nonzero(~passed)[0]
    rec = smp.reshape(-1)[ref["rows"]]
    assert not len(bad), (case, flags, len(bad), [(int(i), int(rec["state"][i]), int(ref["state"][i]), int(rec["second"][i]), int(ref["second"][i]),
                                                    float(rec["pdf"][i]), float(ref["pdf"][i]), bool(ref["aside"][i])) for i in bad[:4]], worst)
    assert share <= lr.EDGE_CAP and light >= 50 and bsdf >= 50 and grazing >= 20
    judged = ~ref["aside"]
    states = rec["state"][judged]
    assert (states == lr.LIGHT).any() and (states == lr.BSDF).any() and (states == lr.ENDED_ZERO).any()
    assert (rec["second"][judged] == lr.SECOND_EMITTER).any() and (rec["second"][judged] == lr.SECOND_SURFACE).any()
    if case == "cornell+sun":
        assert (ref["distant"][judged] > 0).any()
