"""-m gpu: spheres and meshes under general affine maps (tests/transform_cases.py) on every kernel family.  Every sphere the other
GPU tests render is a translation times a uniform radius -- the item loop's ball short form, a diagonal world_to_object -- and every
mesh but one a translation.  Here:

a. Renderer.trace against the fp64 reference and the oracle for every map of the catalogue: item loop, BVH, a deep tree, the emitter
   structure; rays from outside, from inside (the second root), from the surface (the first root below tmin), tangent ones.
b. the queue traversal pass (kernels_gate.hip) on a deep scene with general spheres against rene_trace.
c. the first-hit layers of one frame against the oracle: the normal through the inverse transpose, sphere_uv through an image map.
d. whole renders on every leaf of the dispatch that has FEAT_SPHERES, the launch log naming the kernel, production variants bit
   for bit their counting twin.
e. sphere emitters under rotated, non-uniform and mirrored maps and under one whose quirk radius (Q4) is zero.
f. mesh emitters under non-uniform, sheared and mirrored maps; one mesh instanced three times.

Which one-line mutation of the device code or the packer fails which of these tests: DESIGN.md, section 2."""
import numpy as np
import pytest

import kernel_matrix as km
import transform_cases as tc
from rene_amd import abi, api
from test_gpu_kernel_matrix import _against_the_oracle, _oracle, _render, log  # noqa: F401 (log: a fixture)
from test_gpu_parity import aov_check
from test_transform_cases import check_every_map_is_judged, gallery_rays

pytestmark = pytest.mark.gpu


# ---- a. intersection ------------------------------------------------------------------------------------------------------------------
TRACE = {"item-loop": (False, 0, 0), "bvh": (False, abi.FLAG_FORCE_BVH, 0), "deep": (True, 0, 0),
         "item-loop-emitters": (False, 0, 1), "bvh-emitters": (False, abi.FLAG_FORCE_BVH, 1), "deep-emitters": (True, 0, 1)}


@pytest.mark.parametrize("mode", list(TRACE))
def test_trace_against_the_fp64_reference(mode, oracle_mod):
    """Hit or miss, instance and primitive equal the fp64 reference's and t lies within the project's 5e-5 / 5e-5 of it on every ray
    that is not grazing (transform_cases: |disc| / half_b^2 < 1e-3, roots within 1e-2 of each other or 2e-4 of tmin, a triangle's
    edge within 2e-4, its plane within 1e-2 of the ray, a second surface within twice the margin): at most 2 % of the rays by the
    reference alone, and every map keeps more than 600 judged hits.  Against the oracle: as test_traversal_matches_oracle."""
    deep, flags, which = TRACE[mode]
    s, o, d, refs = gallery_rays(deep)
    ref = refs[which]
    if which == 0:
        check_every_map_is_judged(s, ref)
    assert ref["grazing"].mean() <= 0.02
    info = api.pack_info(s)
    assert bool(info.features & km.SMALL) == (not deep) and (not deep or info.n_nodes_main > km.RESTART_MIN_NODES)
    with api.Renderer(s, flags=flags) as r:
        hg = r.trace(o, d, which=which)
    n = tc.compare_hits(hg, ref, mode)
    print(f"{mode}: {n} of {len(o)} rays judged, {int(ref['grazing'].sum())} grazing")
    assert n >= 0.98 * len(o)
    assert tc.compare_points(hg, ref, s) > 100
    ho = oracle_mod.Oracle(s).trace(o, d, which=which)
    keep = ~ref["grazing"]
    assert np.array_equal(hg["t"][keep] < 0, ho["t"][keep] < 0)
    both = keep & (ho["t"] > 0)
    assert np.array_equal(hg["instance"][both], ho["instance"][both]) and np.array_equal(hg["primitive"][both], ho["primitive"][both])
    np.testing.assert_allclose(hg["t"][both], ho["t"][both], rtol=5e-5, atol=5e-5)


# ---- b. the queue pass ----------------------------------------------------------------------------------------------------------------
def test_the_queue_traversal_pass_on_general_spheres():
    """rene_trace_queue (kernels_gate.hip) on the deep gallery: its sphere branch runs intersect_sphere through a full world_to_object.
    Closest-hit rays find the hit rene_trace finds, bit for bit; any-hit rays the same verdict; rays flagged for the emitter structure
    what rene_trace(which = 1) finds."""
    s, o, d, refs = gallery_rays(True)
    n = len(o)
    rng = np.random.default_rng(3)
    any_hit = (rng.random(n) < 0.3).astype(np.uint32)
    emit = (rng.random(n) < 0.3).astype(np.uint32)
    flag_words = (any_hit | (emit << 1)).astype(np.uint32)
    o_tmax = np.ascontiguousarray(np.concatenate([o, np.full((n, 1), 1e5, np.float32)], axis=1))
    d32 = np.ascontiguousarray(np.concatenate([d, flag_words.view(np.float32)[:, None]], axis=1))
    with api.Renderer(s, flags=abi.FLAG_COUNTERS) as r:
        ref = [r.trace(o, d, 0.001, 1e5, w) for w in (0, 1)]
        want_t = np.where(emit == 1, ref[1]["t"], ref[0]["t"])
        sphere_hits = sum(int(((ref[0]["t"] > 0) & (ref[0]["instance"] == i)).sum()) for i, inst in enumerate(s.instances) if inst.shape == abi.SHAPE_SPHERE)
        assert sphere_hits > 6000
        for refill in (1, 16, 64):
            _, hits, steps = r.trace_queue(o_tmax, d32, False, refill, 6, 0, 1, True, True)
            assert np.array_equal(hits[:, 0] < 0, want_t < 0), refill
            closest = any_hit == 0
            assert np.array_equal(hits[closest, 0], want_t[closest]), refill
            assert steps[1] > 0 and steps[3] > 0


# ---- c. first-hit layers --------------------------------------------------------------------------------------------------------------
def _first_hit(s, oracle_mod, log, monkeypatch, textured, dispatches, self_pixels=(0, 0)):
    """One frame: layers 1 and 2 against the oracle's at the project's atol 5e-5 x frames (aov_check; a camera ray that grazes a
    silhouette may land on the other side: 2e-3 of the pixels, its default).  A sphere's normal towards its limb is ill-conditioned in
    fp32 whoever computes it: the oracle's two builds differ beyond 5e-5 in `self_pixels` pixels (transform_cases.SELF_FIRST_HIT:
    8 for the translated ball, 61 under `nonuniform`), and the device may in transform_cases.pixel_bound of them -- on a film where a
    normal from the wrong matrix moves the 200 to 500 pixels the spheres cover (device, measured: 10, 9, 71, 8, 33, 9, 5, 9, 10 in
    the order of the catalogue).  Where a Matte over the 7 x 5 image map is in view the
    albedo takes the bound of test_image_map_repeats_over_many_periods, 6e-3 per frame on all but 2 % of the pixels and the mean within
    2e-3: there a hit's barycentrics, good to 2e-5, move the look-up by 1e-3 of a texel (8 periods of 7 texels across the quad); here
    a hit point good to 5e-5 on a sphere of semi-axes 0.15 and more moves sphere_uv by 3e-4 rad, 7 / (2 pi) texels per rad: 4e-4 of a
    texel (more within a few pixels of the poles) -- while a uv from the wrong axes lands on another texel: ~ 0.3."""
    o = oracle_mod.Oracle(s)
    o.render(0, 1)
    ref = [o.download(l) for l in range(3)]
    assert (np.abs(ref[1]).sum(axis=2) > 0).mean() > 0.5
    info = api.pack_info(s)
    for flags in dispatches:
        km.read_log(log)
        with api.Renderer(s, flags=flags) as r:
            r.render(0, 1)
            g = [r.download(l) for l in range(3)]
        names = km.read_log(log)
        if flags & abi.FLAG_WAVEFRONT:
            assert names == [], (flags, names)  # the context took the scene: the wavefront integrator launches no megakernel
        else:
            assert names == [km.expected_kernel(info, flags)], (flags, names)
        d1 = np.abs(g[1] - ref[1]).max(axis=2)
        print(f"flags {flags}: normal layer, pixels beyond 5e-5: {int((d1 > 5e-5).sum())}, albedo: {int((np.abs(g[2] - ref[2]).max(axis=2) > 5e-5).sum())}")
        aov_check(g[1], ref[1], atol=5e-5, frac=tc.pixel_bound(self_pixels[0], 2e-3))
        if textured:
            aov_check(g[2], ref[2], atol=6e-3, frac=2e-2)
            assert abs(float(g[2].mean()) - float(ref[2].mean())) <= 2e-3 * float(ref[2].mean())
        else:
            aov_check(g[2], ref[2], atol=5e-5, frac=tc.pixel_bound(self_pixels[1], 2e-3))


SMALL_DISPATCHES = (0, abi.FLAG_FORCE_BVH, abi.FLAG_FORCE_BVH | abi.FLAG_WAVEFRONT)
DEEP_DISPATCHES = (0, abi.FLAG_FORCE_BVH, abi.FLAG_NO_RESTART, abi.FLAG_WAVEFRONT)


@pytest.mark.parametrize("name", tc.MAPS)
def test_first_hit_layers_of_spheres(name, oracle_mod, log, monkeypatch):
    """shade_hit_lds (item loop) and shade_hit (BVH, wavefront): the normal from the columns of world_to_object, sphere_uv of the
    object-space hit point under an image map, for a textured Matte, a Glass and a Mirror sphere under every map."""
    _first_hit(tc.first_hit_spheres(name), oracle_mod, log, monkeypatch, True, SMALL_DISPATCHES, tc.SELF_FIRST_HIT[name])


@pytest.mark.parametrize("smooth", [True, False], ids=["smooth", "flat"])
@pytest.mark.parametrize("name", ["nonuniform", "sheared", "mirrored"])
def test_first_hit_layers_of_meshes(name, smooth, oracle_mod, log, monkeypatch):
    """The packer's xform_normal(w2o, .) of vertex normals and of the geometric normal where a mesh has none."""
    _first_hit(tc.first_hit_mesh(name, smooth), oracle_mod, log, monkeypatch, False, DEEP_DISPATCHES)


# ---- d. whole renders ---------------------------------------------------------------------------------------------------------------
def _matrix(s, family, leaf, cls, oracle_mod, log, monkeypatch, variants=None, self_pixels=(0, 0, 0)):
    """test_every_instantiation_against_the_oracle_and_its_counting_twin for one scene: returns the kernels logged.  `self_pixels`:
    what the oracle's two builds differ in on this scene (transform_cases.SELF_*); the first-hit layers may differ in
    transform_cases.pixel_bound of the larger of the two layers' counts."""
    info = api.pack_info(s)
    ref, so = _oracle(s, oracle_mod)
    out, logged = {}, set()
    for v in variants or km.VARIANTS[family]:
        g, sg, names = _render(s, v.flags, log, monkeypatch, v.no_lds_tables)
        want = km.expected_kernel(info, v.flags, v.no_lds_tables)
        assert names and set(names) == {want}, (v.name, names, want)
        if leaf is not None:
            assert km.kernel_feat(want) == leaf, (v.name, want)
        logged.add(want)
        if v.twin is None:
            assert np.isfinite(g[0]).all()
            _against_the_oracle(g, sg, ref, so, cls, aov_frac=tc.pixel_bound(max(self_pixels[1:]), 5e-3))
            assert sg["hits"] > 0 and g[0].sum() > 0
        else:
            t, st = out[v.twin]
            assert np.array_equal(g[0], t[0]), (v.name, v.twin, int((g[0] != t[0]).sum()))
            for l in (1, 2):
                if v.flags & abi.FLAG_NO_AOV:
                    assert not g[l].any(), (v.name, l)
                else:
                    assert np.array_equal(g[l], t[l]), (v.name, v.twin, l)
            assert sg["paths"] == st["paths"]
        out[v.name] = (g, sg)
    return logged


@pytest.mark.parametrize("name", [e.name for e in tc.RENDERS])
def test_general_spheres_on_every_leaf_that_has_them(name, oracle_mod, log, monkeypatch):
    """A catalogue scene of the kernel matrix with its spheres, boxes and deep mesh under a map each: 16 frames against the oracle
    with the tolerances of its class (counters, T1, first-hit layers, mean), the launch log naming the leaf's kernel -- for the restart
    families its while-while twin too -- and every production variant equal to its counting twin bit for bit.
    One scene does not fit the matrix's 5e-3 of the pixels for the first-hit layers: plastic-uber-deep/nonuniform, three spheres under
    the map of condition 4, where the oracle's own two builds differ in 42 pixels (1.2 %; transform_cases.SELF_RENDERS) and the
    device differs from the oracle in 39; its bound is pixel_bound(42) = 88 pixels.  Every other scene keeps 5e-3."""
    e = tc.RENDER_BY_NAME[name]
    logged = _matrix(e.build(), e.family, e.leaf, e.cls, oracle_mod, log, monkeypatch, self_pixels=tc.SELF_RENDERS.get(name, (0, 0, 0)))
    assert all(km.kernel_feat(k) & km.SPHERES for k in logged)
    if "restart" in e.family:
        assert any("render_kernel_wf" in k for k in logged) and any("render_kernel_wf" not in k for k in logged)


# ---- e. sphere emitters -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rotated", "nonuniform", "mirrored", "cyclic"])
def test_sphere_emitter_pdf(name, oracle_mod):
    """emitter_pdf on the global tables (rene_emitter_pdf: the item loop and, with FLAG_FORCE_BVH, the BVH) and, on the item-loop context,
    emitter_pdf_lds on the LDS image in both of its forms (rene_emitter_pdf_form 1 and 2), at the same tolerances: the ray meets the
    ellipsoid through the full world_to_object, while the pdf
    is the cone of a sphere whose radius is the mean of the absolute diagonal (quirk Q4) -- the reference wants exactly that.  With the
    quirk radius at least 0.1 of the distance, 1 - cos(theta_max) keeps its bits and the project's 2e-4 holds (the r = 1 row of
    test_emitter_pdf_probe_spheres).  `cyclic`: a zero diagonal, the reference's pdf is 1 / 0 = +inf, and so is the device's, on
    exactly the rays that hit."""
    s = tc.emitter_room(name)
    m = tc.ctm(name, tc.EMITTER_AT, size=tc.EMITTER_SIZE)
    q = tc.quirk_radius(m)
    far = 2.2 if name == "cyclic" else min(2.2, q / 0.1)
    rng = np.random.default_rng(8)
    org, d = tc.emitter_rays(m, rng, 4000, far)
    miss_o, miss_d = tc.emitter_rays(tc.ctm(name, (1.5, 0.4, 1.0), size=tc.EMITTER_SIZE), rng, 400)  # aimed elsewhere: most of them miss
    org, d = np.concatenate([org, miss_o]), np.concatenate([d, miss_d])
    ref = tc.Reference(s, 1).trace(org, d)
    keep = ~ref["grazing"]
    assert keep.mean() >= 0.98 and (ref["t"][keep] > 0).sum() > 3500 and (ref["t"][keep] < 0).sum() > 200
    if name != "cyclic":
        dist = np.linalg.norm(org[:4000].astype(np.float64) - np.float64(tc.EMITTER_AT), axis=1)
        assert q > 0.2 and (q / dist >= 0.1).all()
    f32, _ = oracle_mod.Oracle(s).emitter_pdf(org, d)
    assert np.array_equal(f32[keep] > 0, ref["t"][keep] > 0)  # the oracle hits what the fp64 reference hits
    for flags in (0, abi.FLAG_FORCE_BVH):
        with api.Renderer(s, flags=flags) as r:
            forms = {0: r.emitter_pdf(org, d)}
            if not flags:
                forms.update({form: r.emitter_pdf_form(form, org, d) for form in (1, 2)})
        for form, g in forms.items():
            assert np.array_equal(g[keep] > 0, ref["t"][keep] > 0), (flags, form)
            hit = keep & (ref["t"] > 0)
            if name == "cyclic":
                assert np.isposinf(f32[hit]).all() and np.array_equal(np.isposinf(g), np.isposinf(f32)), (flags, form)
                assert np.array_equal(np.isposinf(g[keep]), hit[keep])
            else:
                rel = np.abs(g[hit] - f32[hit]) / f32[hit]
                print(f"{name}, flags {flags}, form {form}: quirk radius {q:.4f}, device vs oracle max {rel.max():.3g}")
                assert np.isfinite(g).all() and rel.max() <= 2e-4, (flags, form, float(rel.max()))
                true_r = float(np.cbrt(abs(np.linalg.det(m[:3, :3].astype(np.float64)))))
                assert abs(q - true_r) > 0.02 * true_r  # (the quirk is visible: a true radius would be off by far more than 2e-4)


EMITTER_VARIANTS = (km.Variant("count", abi.FLAG_COUNTERS, False, None), km.Variant("aov", 0, False, "count"),
                    km.Variant("bvh-count", abi.FLAG_COUNTERS | abi.FLAG_FORCE_BVH, False, None), km.Variant("bvh-aov", abi.FLAG_FORCE_BVH, False, "bvh-count"))


@pytest.mark.parametrize("name", ["rotated", "nonuniform", "mirrored", "cyclic"])
def test_sphere_emitter_renders(name, oracle_mod, log, monkeypatch):
    """A Matte room lit by one sphere emitter under the map: emit_sample_lds and emitter_pdf_lds on the item loop, emit_sample and
    emitter_pdf with RENE_FLAG_FORCE_BVH, against the oracle; finite also where the pdf is infinite (`cyclic`).
    The Matte class's 1e-3 of the pixels at T1 does not hold for a room lit by a sphere, translated ball or not: the reference samples
    the emitter ON its surface and then meets it with a ray, a tangent one for a sample near the limb.  The oracle's own two builds
    differ in 20 (ball), 28, 29 and 20 pixels (0.6 to 0.8 %; transform_cases.SELF_EMITTERS), the device in 25, 35 and 24: the class
    is kernel_matrix.TOL["sphere-lit"], the 2e-2 and 1e-4 of test_veach_mis_without_the_small_light_is_tight.  `cyclic`, whose
    light-sampling branch weighs nothing, keeps the Matte class."""
    s = tc.emitter_room(name)
    logged = _matrix(s, "item", None, "matte" if name == "cyclic" else "sphere-lit", oracle_mod, log, monkeypatch, EMITTER_VARIANTS,
                     self_pixels=tc.SELF_EMITTERS[name])
    assert any(km.kernel_feat(k) & km.SMALL for k in logged) and any(not km.kernel_feat(k) & km.SMALL for k in logged)
    assert all(km.kernel_feat(k) & km.SPHERES for k in logged)


# ---- f. mesh emitters and instancing ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["quad", "mesh"])
@pytest.mark.parametrize("name", ["nonuniform", "sheared", "mirrored"])
def test_mesh_emitters(name, which, oracle_mod, log, monkeypatch):
    """The triangle-emitter pdf's operands from the packer (the world normal through the inverse transpose over its length, the
    world-space area) at the project's rtol 3e-4 (test_emitter_pdf_probe_triangles), then the render against the oracle."""
    s = tc.mesh_emitter_room(name, which)
    emitter = next(i for i in s.instances if i.area_light_index)
    rng = np.random.default_rng(12)
    org, d = tc.mesh_rays(tc.world_corners(s, emitter), rng, 4000)
    ref = tc.Reference(s, 1).trace(org, d)
    keep = ~ref["grazing"]
    hit = keep & (ref["t"] > 0)
    assert keep.mean() >= 0.98 and hit.sum() > 3000
    f32, _ = oracle_mod.Oracle(s).emitter_pdf(org, d)
    f64 = tc.triangle_emitter_pdf(ref, d, len(tc.world_corners(s, emitter)))
    np.testing.assert_allclose(f32[hit], f64[hit], rtol=3e-4)  # the oracle against the geometry first
    for flags in (0, abi.FLAG_FORCE_BVH):
        with api.Renderer(s, flags=flags) as r:
            forms = {0: r.emitter_pdf(org, d)}
            if not flags and api.pack_info(s).features & km.SMALL:  # the LDS forms of the item-loop context (the quad; the mesh is a BVH scene)
                forms.update({form: r.emitter_pdf_form(form, org, d) for form in (1, 2)})
        assert set(forms) == ({0, 1, 2} if which == "quad" and not flags else {0})
        for form, g in forms.items():
            assert np.array_equal(g[keep] > 0, ref["t"][keep] > 0) and np.array_equal(f32[keep] > 0, ref["t"][keep] > 0), (flags, form)
            rel = np.abs(g[hit] - f32[hit]) / f32[hit]
            print(f"{name} {which}, flags {flags}, form {form}: device vs oracle max {rel.max():.3g} at ray {np.nonzero(hit)[0][rel.argmax()]}")
            np.testing.assert_allclose(g[hit], f32[hit], rtol=3e-4)
            np.testing.assert_allclose(g[hit], f64[hit], rtol=3e-4)
    if which == "quad":
        logged = _matrix(s, "item", None, "matte", oracle_mod, log, monkeypatch, EMITTER_VARIANTS)
        assert any(km.kernel_feat(k) & km.SMALL for k in logged)
    else:
        logged = _matrix(s, "restart", 8, "matte", oracle_mod, log, monkeypatch)
        assert any("render_kernel_wf" in k for k in logged)


def test_one_mesh_instanced_three_times(oracle_mod, log, monkeypatch):
    """add_mesh_instance: one mesh under three maps and three materials.  rene_trace names the instance the fp64 reference names, and
    the render matches the oracle."""
    s, ids = tc.instanced()
    rng = np.random.default_rng(4)
    rays = [tc.mesh_rays(tc.world_corners(s, s.instances[i]), rng, 2000) for i in ids]
    o, d = np.concatenate([r[0] for r in rays]), np.concatenate([r[1] for r in rays])
    ref = tc.Reference(s).trace(o, d)
    assert ref["grazing"].mean() <= 0.02
    for i in ids:
        assert (~ref["grazing"] & (ref["instance"] == i)).sum() > 1000, i
    for flags in (0, abi.FLAG_FORCE_BVH):
        with api.Renderer(s, flags=flags) as r:
            hg = r.trace(o, d)
        assert tc.compare_hits(hg, ref, f"flags {flags}") >= 0.98 * len(o)
        assert tc.compare_points(hg, ref, s) > 3000
    family = "restart" if api.pack_info(s).n_nodes_main > km.RESTART_MIN_NODES else "item"  # (the item family's variants fit any kernel)
    _matrix(s, family, None, "single", oracle_mod, log, monkeypatch)
