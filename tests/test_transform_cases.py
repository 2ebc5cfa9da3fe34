"""Spheres and meshes under general transforms, without a GPU (tests/transform_cases.py): the catalogue of maps, the packer's ball
recogniser at its boundary, the pbrt loader's spheres under a CTM, the transformed scenes' place in the kernel dispatch, and the
oracle -- BVH and brute force -- against the fp64 reference, before either judges the device (test_gpu_transforms.py)."""
import numpy as np
import pytest

import kernel_matrix as km
import transform_cases as tc
from rene_amd import abi, api, glam, loader

KIND_SPHERE, KIND_BALL = 2.0, 4.0  # SMALL_KIND_SPHERE, SMALL_KIND_BALL (csrc/device_scene.h)


def test_the_catalogue_is_what_it_says():
    for name in tc.MAPS:
        m = tc.linear(name).astype(np.float64)
        sv = np.linalg.svd(m, compute_uv=False)
        assert sv.max() / sv.min() <= tc.MAX_CONDITION, name
        assert 0.1 <= sv.min() and sv.max() <= 0.7, name  # the size of the room's spheres
    r = np.float64(tc.linear("uniform")[0, 0])
    assert (np.diag(tc.linear("cyclic")) == 0).all() and tc.quirk_radius(tc.ctm("cyclic")) == 0.0
    assert np.linalg.det(tc.linear("mirrored").astype(np.float64)) < 0 and np.linalg.det(tc.linear("mirrored-uniform").astype(np.float64)) < 0
    assert np.array_equal(tc.linear("mirrored-uniform"), -tc.linear("uniform"))
    for name, lo, hi in (("inside-tolerance", 1e-7, 5e-7), ("outside-tolerance", 2e-6, 8e-6)):  # the recogniser's tolerance is 1e-6 |r|
        m = tc.linear(name).astype(np.float64)
        assert m[0, 0] == r and m[2, 2] == r
        assert lo * r < m[1, 1] - r < hi * r and lo * r < m[1, 0] < hi * r, (name, (m[1, 1] - r) / r, m[1, 0] / r)
    for name in ("rotated", "nonuniform", "sheared", "mirrored"):  # nothing of these is near a ball: every entry matters
        m = tc.linear(name)
        assert np.abs(m).min() > 0.01


def _one_sphere(name):
    s = km.room()
    s.add_sphere(1.0, s.add_matte((0.5, 0.5, 0.5)), ctm=tc.ctm(name, (0.3, 0.7, -0.4)))
    return s


def _sphere_kinds(scene):
    items, n_loop = api.small_items(scene, 0)
    kinds = items[:n_loop, 12].view(np.float32)
    return kinds[(kinds == KIND_SPHERE) | (kinds == KIND_BALL)]


@pytest.mark.parametrize("name", tc.MAPS)
def test_the_ball_recogniser_at_its_boundary(hip_lib, name):
    """Translation + positive uniform scale (to 1e-6 of the radius) is the item loop's short form; everything else, `-r` on all three
    axes and a rotation whose diagonal is zero included, is the general sphere item.  FEAT_SPHERES either way."""
    s = _one_sphere(name)
    info = api.pack_info(s)
    assert info.features & km.SPHERES and info.features & km.SMALL and info.n_spheres == 1
    assert _sphere_kinds(s).tolist() == [KIND_BALL if name in tc.BALLS else KIND_SPHERE]


def test_a_sphere_as_scene_builders_place_it_is_a_ball(hip_lib):
    s = km.room(["metal"], spheres=True)
    assert _sphere_kinds(s).tolist() == [KIND_BALL]


PBRT = '''
LookAt 0 1 -5  0 0.7 0  0 1 0
Camera "perspective" "float fov" 38
WorldBegin
LightSource "infinite" "rgb L" [1 1 1]
AttributeBegin
  Translate 0.2 0.65 -0.6
  Rotate 40 0 0 1
  Scale 1 2 0.5
  Shape "sphere" "float radius" 0.3
AttributeEnd
AttributeBegin
  Translate -1 0.3 0.25
  Shape "sphere" "float radius" 0.3
AttributeEnd
AttributeBegin
  Translate 1 0.5 0.25
  Rotate 120 0.57735026 0.57735026 0.57735026
  Shape "sphere" "float radius" 0.25
AttributeEnd
WorldEnd
'''


def test_the_loader_multiplies_the_whole_ctm_into_a_sphere(hip_lib):
    """pbrt_loader.cpp: a sphere's matrix is CTM x scale(radius) -- Rotate and Scale ahead of Shape "sphere" included -- and such a sphere
    is the general item; a sphere under a Translate alone is the ball."""
    s = loader.parse_pbrt(PBRT)
    assert s.desc.n_instances == 3
    f32 = np.float32
    deg = lambda a: float(f32(f32(a) * f32(np.pi)) / f32(180.0))  # deg_to_radian in float
    axis = np.float32([0.57735026] * 3).astype(np.float64)
    axis = (axis / np.sqrt((axis * axis).sum())).astype(np.float32)
    want = [glam.mul(glam.mul(glam.mul(glam.from_translation((0.2, 0.65, -0.6)), glam.from_axis_angle((0, 0, 1), deg(40))),
                              glam.from_scale((1, 2, 0.5))), glam.from_scale((0.3,) * 3)),
            glam.mul(glam.from_translation((-1, 0.3, 0.25)), glam.from_scale((0.3,) * 3)),
            glam.mul(glam.mul(glam.from_translation((1, 0.5, 0.25)), glam.from_axis_angle(axis, deg(120))), glam.from_scale((0.25,) * 3))]
    for k in range(3):
        inst = s.desc.instances[k]
        assert inst.shape == abi.SHAPE_SPHERE
        np.testing.assert_allclose(np.array(inst.matrix[:], np.float32), glam.affine_from_mat4(want[k]), rtol=2e-7, atol=3e-8, err_msg=str(k))
    m = np.array(s.desc.instances[0].matrix[:9]).reshape(3, 3).T
    assert abs(m[0, 1]) > 0.3 and abs(m[1, 1] / m[0, 0]) > 1.9  # rotated and non-uniform indeed
    assert sorted(_sphere_kinds(s).tolist()) == [KIND_SPHERE, KIND_SPHERE, KIND_BALL]
    assert api.pack_info(s).features & km.SPHERES
    head, *blocks = PBRT.split("AttributeBegin")  # (items come in the order of the tree's slots: one sphere at a time says which is which)
    for block, kind in zip(blocks, (KIND_SPHERE, KIND_BALL, KIND_SPHERE)):
        one = loader.parse_pbrt(head + "AttributeBegin" + block + ("" if "WorldEnd" in block else "WorldEnd\n"))
        assert one.desc.n_instances == 1 and _sphere_kinds(one).tolist() == [kind]


def test_the_transformed_scenes_reach_their_leaves(hip_lib):
    """Every transformed scene of the render tests takes the leaf of the catalogue entry it was made from, every leaf with FEAT_SPHERES
    is among them, and in the item-loop families the spheres are general items (no ball among them)."""
    leaves = set()
    for e in tc.RENDERS:
        s = e.build()
        info = api.pack_info(s)
        assert km.kernel_feat(km.expected_kernel(info)) == e.leaf and e.leaf & km.SPHERES, e.name
        assert bool(info.n_nodes_main > km.RESTART_MIN_NODES) == ("restart" in e.family), e.name
        leaves.add((e.family, e.leaf))
        if info.features & km.SMALL:
            kinds = _sphere_kinds(s)
            assert len(kinds) == info.n_spheres and (kinds == KIND_SPHERE).all(), e.name
    want = {(e.family, e.leaf) for e in km.CATALOGUE if e.leaf & km.SPHERES}
    assert leaves == want == {("item", 835), ("item", 67), ("item", 95), ("item", 127), ("restart", 31), ("restart", 63),
                              ("vol-item", 223), ("vol-item", 255), ("vol-restart", 159), ("vol-restart", 191)}
    for name in tc.MAPS:
        assert api.pack_info(tc.first_hit_spheres(name)).features & km.SMALL
    for name in ("nonuniform", "sheared", "mirrored"):
        assert api.pack_info(tc.first_hit_mesh(name, True)).n_nodes_main > km.RESTART_MIN_NODES
        assert api.pack_info(tc.emitter_room(name)).features & km.SMALL
        assert api.pack_info(tc.mesh_emitter_room(name, "quad")).features & km.SMALL
        assert api.pack_info(tc.mesh_emitter_room(name, "mesh")).n_nodes_main > km.RESTART_MIN_NODES
    small, deep = api.pack_info(tc.gallery()), api.pack_info(tc.gallery(deep=True))
    assert small.features & km.SMALL and deep.n_nodes_main > km.RESTART_MIN_NODES and not deep.features & km.SMALL


# ---- the fp64 reference against closed forms ------------------------------------------------------------------------------------------
def test_the_fp64_sphere_against_closed_forms():
    o = np.array([[0.0, 0.0, -5.0], [0.0, 0.0, 0.0], [0.0, 0.0, -2.0], [0.0, 3.0, -5.0], [2.5, 0.0, -5.0]])
    d = np.array([[0.0, 0.0, 1.0]] * 5)
    m = np.diag([2.0, 3.0, 2.0, 1.0])  # semi-axes 2, 3, 2 about the origin
    t, n, disc_n, roots = tc.ray_sphere(m, o, d)
    assert np.allclose(t[:3], [3.0, 2.0, 4.0])      # from outside: the first root; from the centre and from the surface: the second
    assert np.isnan(t[4]) and disc_n[4] < 0           # past it
    assert abs(disc_n[3]) < 1e-12 and np.allclose(roots[3], 5.0)  # tangent at the tip of the long axis
    assert np.allclose(n[0] / np.linalg.norm(n[0]), [0, 0, -1]) and np.allclose(n[1] / np.linalg.norm(n[1]), [0, 0, 1])
    # a sheared sphere: the normal is perpendicular to the surface's tangents, M t, for every tangent t of the unit sphere at p
    m = tc.ctm("sheared", (0.3, -0.2, 0.1)).astype(np.float64)
    rng = np.random.default_rng(0)
    oo, dd = tc.sphere_rays(m, rng, 400)
    t, n, _, _ = tc.ray_sphere(m, oo.astype(np.float64), dd.astype(np.float64))
    hit = ~np.isnan(t)
    p = (oo.astype(np.float64) + t[:, None] * dd)[hit]
    p_obj = (p - m[:3, 3]) @ np.linalg.inv(m[:3, :3]).T
    assert hit.sum() > 300 and np.allclose(np.linalg.norm(p_obj, axis=1), 1.0, atol=1e-6)  # (the rays are float32 numbers: t is exact for them)
    tangent = np.cross(p_obj, rng.normal(size=p_obj.shape)) @ m[:3, :3].T
    assert np.abs((tangent * n[hit]).sum(1)).max() < 1e-9


def test_the_fp64_triangle_against_closed_forms():
    corners = np.array([[[0.0, 0.0, 1.0], [2.0, 0.0, 1.0], [0.0, 4.0, 1.0]], [[0.0, 0.0, 3.0], [2.0, 0.0, 3.0], [0.0, 4.0, 3.0]]])
    o = np.array([[0.5, 1.0, -1.0], [0.5, 1.0, 2.0], [1.5, 3.5, -1.0], [0.5, 1.0, 5.0]])
    d = np.array([[0.0, 0.0, 1.0]] * 3 + [[0.0, 0.0, -2.0]])
    t, u, v, k, n = tc.ray_triangles(corners, o, d)
    assert np.allclose(t[[0, 1, 3]], [2.0, 1.0, 1.0]) and k.tolist() == [0, 1, -1, 1] and np.isnan(t[2])
    assert np.allclose(u[[0, 1, 3]], 0.25) and np.allclose(v[[0, 1, 3]], 0.25) and np.allclose(n[0], [0, 0, 8])


# ---- the oracle against the fp64 reference -------------------------------------------------------------------------------------------
_RAYS = {}


def gallery_rays(deep):
    """(scene, origins, directions, {which: Reference.trace}) of a gallery: computed once, shared, left unchanged."""
    if deep not in _RAYS:
        s = tc.gallery(deep=deep)
        o, d = tc.probe_rays(s, seed=11 + deep)
        _RAYS[deep] = (s, o, d, {w: tc.Reference(s, w).trace(o, d) for w in (0, 1)})
    return _RAYS[deep]


def check_every_map_is_judged(s, ref):
    """by the fp64 reference alone: at most 2 % of the rays are grazing, and every sphere is hit by plenty of rays that are not"""
    assert ref["grazing"].mean() <= 0.02, ref["grazing"].mean()
    for i, inst in enumerate(s.instances):
        if inst.shape == abi.SHAPE_SPHERE:
            assert (~ref["grazing"] & (ref["t"] > 0) & (ref["instance"] == i)).sum() > 600, i


@pytest.mark.parametrize("which", [0, 1], ids=["main", "emitters"])
@pytest.mark.parametrize("deep", [False, True], ids=["small", "deep"])
def test_the_oracle_against_the_fp64_reference(oracle_mod, deep, which):
    """Oracle.trace equals its own brute force, and both equal the fp64 reference -- hit or miss, instance, primitive, t within the
    project's 5e-5 / 5e-5, the point that u and v name within the same -- on every ray that is not grazing (transform_cases.GRAZING_DISC, EDGE, PARALLEL)."""
    s, o, d, refs = gallery_rays(deep)
    ref = refs[which]
    check_every_map_is_judged(s, ref)
    orc = oracle_mod.Oracle(s)
    ho, hb = orc.trace(o, d, which=which), orc.trace(o, d, which=which, bruteforce=True)
    assert np.array_equal(ho["t"], hb["t"])
    hit = ho["t"] > 0
    assert np.array_equal(ho["instance"][hit], hb["instance"][hit]) and np.array_equal(ho["primitive"][hit], hb["primitive"][hit])
    for h, what in ((ho, "oracle"), (hb, "brute force")):
        assert tc.compare_hits(h, ref, what) > 0.98 * len(o)
        assert tc.compare_points(h, ref, s) > (1000 if which == 0 else 100)


# ---- what fp32 does to the reference's own formulas -----------------------------------------------------------------------------------
from test_oracle_fp_sensitivity import fma_oracle  # noqa: E402,F401 (a fixture: the oracle built with its multiply-adds contracted)


def _layers(lib, scene, frames):
    import ctypes as C
    p = scene.to_desc()
    h = C.c_void_p()
    assert lib.oracle_create(p.byref(), C.byref(h)) == 0
    lib.oracle_render(h, abi.DEFAULT_SEED, 0, frames, 16, 0, 0, 1)
    out = []
    for layer in range(3):
        a = np.empty((p.yres, p.xres, 3), np.float32)
        lib.oracle_download(h, layer, 3, a.ctypes.data_as(C.c_void_p), a.size)
        out.append(a)
    lib.oracle_destroy(h)
    return out


def _self_pixels(fma, base, scene, frames):
    a, b = _layers(base, scene, frames), _layers(fma, scene, frames)
    t1 = int((np.abs(a[0] - b[0]) > 1e-2 * (1 + np.abs(b[0]))).any(axis=-1).sum())
    return (t1,) + tuple(int((np.abs(a[l] - b[l]).max(axis=2) > 5e-5 * frames).sum()) for l in (1, 2))


def test_the_recorded_self_perturbation_of_the_oracle(fma_oracle, oracle_mod):  # noqa: F811
    """transform_cases.SELF_*: the pixels in which the oracle differs from its own FMA-contracted build, which bound what the device may
    differ in where the project's fractions do not fit.  Measured again: within a third (and 3 pixels) of what is recorded -- another
    compiler contracts other multiply-adds."""
    base = oracle_mod.lib()
    near = lambda got, want: abs(got - want) <= want / 3 + 3
    for name, want in tc.SELF_FIRST_HIT.items():
        got = _self_pixels(fma_oracle, base, tc.first_hit_spheres(name), 1)
        assert near(got[1], want[0]) and near(got[2], want[1]), (name, got, want)
    for name, want in tc.SELF_RENDERS.items():
        got = _self_pixels(fma_oracle, base, tc.RENDER_BY_NAME[name].build(), 16)
        assert all(near(g, w) for g, w in zip(got, want)), (name, got, want)
    for name, want in tc.SELF_EMITTERS.items():
        got = _self_pixels(fma_oracle, base, tc.emitter_room(name), 16)
        assert all(near(g, w) for g, w in zip(got, want)), (name, got, want)
    for name in ("sheared", "mirrored"):  # and where nothing is recorded there is nothing: the meshes
        for smooth in (True, False):
            assert max(_self_pixels(fma_oracle, base, tc.first_hit_mesh(name, smooth), 1)) <= 1
