"""Test helper (not a conftest): one scene per leaf of the render-kernel dispatch, and `expected_kernel`, a restatement of the
host's kernel selection (rene_amd/csrc/kernel_select.h), written independently of it, family by family as the three launcher units
used to dispatch (kernels.hip, kernels_bvh.hip, kernels_vol.hip).  A build lists every render_kernel / render_kernel_wf instantiation in rene_amd/csrc/<unit>.res;
test_kernel_matrix_catalogue.py checks on the CPU that CATALOGUE x VARIANTS reaches every one of them, test_kernel_select.py
checks the selection against this restatement over all of its inputs, and
test_gpu_kernel_matrix.py renders each against the oracle and checks this restatement against the launch log
(RENE_TEST_KERNEL_LOG, kernels.h)."""
import os
import re
from typing import Callable, NamedTuple, Optional

import numpy as np

from rene_amd import abi, glam, scenes
from rene_amd.scene import Scene, TriangleMesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rene_amd", "csrc")
RES_UNITS = ("kernels", "kernels_bvh", "kernels_vol", "kernels_wave", "kernels_gate")

W, H = 77, 45  # ragged against the 8 x 8 micro-tile and the 32 x 32 tile in both axes (3 x 2 tiles)

# scene feature bits (device_scene.h)
SPHERES, GENERAL, TEXTURES, LIGHTS, BACKGROUND, MULTI, SMALL, VOLPATH = 1, 2, 4, 8, 16, 32, 64, 128
NO_SPECULAR, NO_BLEND, NO_MICROFACET, NO_EMITTERS = 256, 512, 1024, 2048
ALL = SPHERES | GENERAL | TEXTURES | LIGHTS | BACKGROUND | MULTI
GEN1 = ALL & ~MULTI

BLOCK = 256                        # device_code.inc
INST_BYTES, LIGHT_BYTES = 96, 32   # sizeof(Inst), sizeof(Light), device_scene.h
LDS_TABLES_MAX = 40 * 1024         # kernel_select.h: stack + instance and light tables within a quarter of a CU's LDS
RESTART_MIN_NODES = 512            # kernel_select.h: deeper trees take the traversal-restart kernel


def mangle(feat: int, maxl: int, bools, wf: bool) -> str:
    """The Itanium name of render_kernel<feat, maxl, bools...> (or render_kernel_wf), as `Function Name:` in *.res prints it."""
    name = "render_kernel_wf" if wf else "render_kernel"
    args = f"Lj{feat}ELi{maxl}E" + "".join(f"Lb{int(bool(b))}E" for b in bools)
    return f"_ZN4rene{len(name)}{name}I{args}EEvNS_9SceneViewENS_12RenderParamsE"


def stack_entries(info) -> int:
    """rene_hip.cpp plan_context: traversal stack entries per lane (RENE_STACK_ENTRIES not set)."""
    depth, stack = max(info.depth_main, info.depth_emit), 16
    while stack < depth:
        stack += 4
    return stack


def expected_kernel(info, flags: int = 0, no_lds_tables: bool = False) -> str:
    """The kernel rene_render launches for a scene with this rene_pack_info under these context flags (RENE_NO_LDS_TABLES set
    or not)."""
    f = info.features & ~(SMALL if flags & abi.FLAG_FORCE_BVH else 0)
    count = bool(flags & abi.FLAG_COUNTERS)
    aov = not flags & abi.FLAG_NO_AOV
    restart = not flags & abi.FLAG_NO_RESTART and info.n_nodes_main > RESTART_MIN_NODES
    if f & VOLPATH:  # the volumetric integrator (kernels_vol.hip)
        if not f & (SPHERES | GENERAL | TEXTURES | BACKGROUND | MULTI):
            feat, maxl = LIGHTS | VOLPATH, 1
        elif not f & MULTI:
            feat, maxl = GEN1 | VOLPATH, 1
        else:
            feat, maxl = ALL | VOLPATH, 5
        if f & SMALL:
            return mangle(feat | SMALL, maxl, (count or aov,) * 2, False)
        if restart:
            return mangle(feat, maxl, (count, count or aov, False), True)
        return mangle(feat, maxl, (count or aov,) * 2, False)
    if not f & SMALL:  # the path integrator over the BVH (kernels_bvh.hip)
        if not f & (SPHERES | GENERAL | TEXTURES | BACKGROUND | MULTI):
            feat, maxl = LIGHTS | (f & NO_EMITTERS), 1
        elif not f & (MULTI | SPHERES | LIGHTS):
            sub = f & NO_SPECULAR and f & NO_MICROFACET  # Substrate the only general material
            feat = GENERAL | TEXTURES | BACKGROUND | ((NO_SPECULAR | NO_MICROFACET | (f & NO_EMITTERS)) if sub else 0)
            maxl = 1
        elif not f & MULTI:
            feat, maxl = GEN1, 1
        else:
            feat, maxl = ALL, 5
        if not restart:  # the while-while kernel has no instantiation with FEAT_NO_EMITTERS
            return mangle(feat & ~NO_EMITTERS, maxl, (count or aov,) * 2, False)
        tables = info.n_instances * INST_BYTES + info.lights_len * LIGHT_BYTES
        lds_tables = (not count and aov and info.n_instances > 0 and not no_lds_tables
                      and stack_entries(info) * BLOCK * 4 + tables <= LDS_TABLES_MAX)
        return mangle(feat, maxl, (count, count or aov, lds_tables), True)
    # the path integrator over the wave-coherent item loop (kernels.hip)
    if not f & (SPHERES | GENERAL | TEXTURES | BACKGROUND | MULTI | LIGHTS):
        feat, maxl = SMALL, 1
    elif not f & (SPHERES | GENERAL | TEXTURES | BACKGROUND | MULTI):
        feat, maxl = LIGHTS | SMALL, 1
    elif not f & (MULTI | TEXTURES | LIGHTS | BACKGROUND):
        feat = SPHERES | GENERAL | SMALL | ((NO_SPECULAR | NO_BLEND) if f & NO_SPECULAR and f & NO_BLEND else 0)
        maxl = 1
    elif not f & MULTI:
        feat, maxl = GEN1 | SMALL, 1
    else:
        feat, maxl = ALL | SMALL, 5
    return mangle(feat, maxl, (count, count or aov), False)


def kernel_feat(name: str) -> int:
    return int(re.search(r"ILj(\d+)E", name).group(1))


def res_kernel_names():
    """Every render_kernel* instantiation the build compiled (rene_amd/csrc/<unit>.res), or None if a .res file is missing."""
    names = set()
    for u in RES_UNITS:
        path = os.path.join(CSRC, u + ".res")
        if not os.path.exists(path):
            return None
        names |= {n for n in re.findall(r"Function Name: (\S+)", open(path).read()) if "render_kernel" in n}
    return names


def read_log(path: str) -> list:
    """The kernel names a RENE_TEST_KERNEL_LOG file holds, in launch order; the file is removed."""
    if not os.path.exists(path):
        return []
    names = open(path).read().split()
    os.remove(path)
    return names


# ---- variants --------------------------------------------------------------------------------------------------------
class Variant(NamedTuple):
    name: str
    flags: int            # context flags
    no_lds_tables: bool   # RENE_NO_LDS_TABLES set
    twin: Optional[str]   # the counting variant whose layers this one must equal bit for bit (None: compared with the oracle)


_C, _N, _R = abi.FLAG_COUNTERS, abi.FLAG_NO_AOV, abi.FLAG_NO_RESTART
VARIANTS = {
    "item": (Variant("count", _C, False, None), Variant("aov", 0, False, "count"), Variant("no-aov", _N, False, "count")),
    "restart": (Variant("count", _C, False, None), Variant("aov", 0, False, "count"), Variant("aov-global-tables", 0, True, "count"),
                Variant("no-aov", _N, False, "count"),
                Variant("ww-count", _C | _R, False, None), Variant("ww-no-aov", _N | _R, False, "ww-count")),
}
VARIANTS["vol-item"] = VARIANTS["item"]
VARIANTS["vol-restart"] = tuple(v for v in VARIANTS["restart"] if v.name != "aov-global-tables")  # (no tables in LDS there)

# tolerances against the oracle (fraction of pixels off at T1, relMSE, counters) as the existing tests justify them per class:
# Matte (test_gpu_scenes, dragon-class), general single-lobe (teapot-class), multi-lobe and Glass (the material zoo), volpath
# (test_gpu_volpath, the restart kernel), Matte rooms lit by a sphere emitter (test_veach_mis_without_the_small_light_is_tight's pixels and
# relMSE: a sample near the emitter's limb is a tangent ray, transform_cases.SELF_EMITTERS; the Matte class's counters)
TOL = {"matte": (1e-3, 1e-4, 5e-4), "single": (5e-3, 1e-3, 2e-3), "multi": (1e-2, 2e-3, 3e-3), "vol": (5e-3, 1e-3, 2e-3),
       "sphere-lit": (2e-2, 1e-4, 5e-4)}


# ---- scenes -----------------------------------------------------------------------------------------------------------
def _quad(p):
    return TriangleMesh.from_arrays(np.float32(p), np.uint32([0, 1, 2, 0, 2, 3]), uvs=scenes._QUAD_UV)


def _material(s, kind):
    return {"matte": lambda: s.add_matte((0.6, 0.55, 0.5)),
            "metal": lambda: s.add_metal(scenes._VEACH_ETA, scenes._VEACH_K, 0.15, 0.08, remap_roughness=False),
            "glass": lambda: s.add_glass(1.5),
            "mirror": lambda: s.add_mirror((0.9, 0.85, 0.8)),
            "image": lambda: s.add_matte(s.add_texture_image_map(np.random.default_rng(5).random((5, 7, 3), dtype=np.float32))),
            "substrate": lambda: s.add_substrate((0.6, 0.3, 0.2), (0.05, 0.05, 0.05), 0.02, 0.02, remap_roughness=False),
            "plastic": lambda: s.add_plastic((0.2, 0.5, 0.3), (0.3, 0.3, 0.3), 0.15),
            "uber": lambda: s.add_uber(kd=(0.3, 0.3, 0.6), ks=(0.2, 0.2, 0.2), kr=(0.1, 0.1, 0.1), kt=(0.3, 0.3, 0.3),
                                       opacity=(0.7, 0.7, 0.7), rough_u=0.1, rough_v=0.2, eta=1.4)}[kind]()


def room(kinds=(), *, spheres=False, deep=None, emitter="quad", sun=False, sky=False, textures=False, volpath=False, ctm=None):
    """A floor and two Matte walls, a box of each material in `kinds` (and a sphere of each with `spheres`), and with `deep` a
    3 520-triangle displaced sphere of that material: a main BVH of about 900 nodes.  Lights: `emitter` "quad" (a triangle emitter
    under the ceiling), "mesh" (an emissive displaced sphere of 3 520 triangles, the only light) or None; `sun` a distant light;
    `sky` a constant infinite light.  `volpath`: Integrator "volpath", a fog filling the room and a dense medium inside it, each
    behind a None-material box (a None sphere would set FEAT_SPHERES).  `ctm` (tests/transform_cases.py): 4 x 4 matrices by ("box", i),
    ("sphere", i) and "deep" that replace the placement of the i-th box (then a 0.6 x 0.9 x 0.5 block about the origin), of the i-th
    sphere (then the unit sphere) and of the deep mesh; what has no entry is placed as ever."""
    ctm = ctm or {}
    s = Scene.new()
    if volpath:
        s.integrator = abi.INTEGRATOR_VOLPATH
    s.set_camera(glam.look_at_lh((0.0, 1.0, -5.0), (0.0, 0.7, 0.0), (0.0, 1.0, 0.0)), 38.0, W, H)
    if textures:
        dark, light = s.add_texture_solid((0.2, 0.2, 0.25)), s.add_texture_solid((0.75, 0.72, 0.66))
        floor = s.add_matte(s.add_texture_checkerboard(dark, light, 6.0, 6.0))
    else:
        floor = s.add_matte((0.72, 0.7, 0.66))
    wall = s.add_matte((0.5, 0.3, 0.25))
    s.add_triangle_mesh(_quad([[-2.5, 0, -2.5], [-2.5, 0, 2.5], [2.5, 0, 2.5], [2.5, 0, -2.5]]), floor)
    s.add_triangle_mesh(_quad([[-2.5, 0, 2.5], [-2.5, 2.5, 2.5], [2.5, 2.5, 2.5], [2.5, 0, 2.5]]), wall)
    s.add_triangle_mesh(_quad([[-2.5, 0, -2.5], [-2.5, 2.5, -2.5], [-2.5, 2.5, 2.5], [-2.5, 0, 2.5]]), wall)
    mats = {k: _material(s, k) for k in dict.fromkeys(tuple(kinds) + ((deep,) if deep else ()))}
    for i, k in enumerate(kinds):
        x = -1.5 + 3.0 * (i + 0.5) / len(kinds)
        if ("box", i) in ctm:
            s.add_triangle_mesh(scenes._aabb((-0.3, -0.45, -0.25), (0.3, 0.45, 0.25)), mats[k], ctm=ctm["box", i])
        else:
            s.add_triangle_mesh(scenes._aabb((x - 0.3, 0.0, 0.9), (x + 0.3, 0.9, 1.4)), mats[k])
        if spheres and ("sphere", i) in ctm:
            s.add_sphere(1.0, mats[k], ctm=ctm["sphere", i])
        elif spheres:
            s.add_sphere(0.3, mats[k], ctm=glam.from_translation((x, 0.3, -0.6)))
    if deep:
        s.add_triangle_mesh(scenes.displaced_sphere(40, 44, radius=0.5, amplitude=0.12, seed=5), mats[deep],
                            ctm=ctm.get("deep", glam.from_translation((0.5, 0.62, 0.2))))
    fog = 0
    if volpath:
        fog = s.add_medium_homogeneous((0.01, 0.01, 0.015), (0.2, 0.2, 0.22), 0.35)
        dense = s.add_medium_homogeneous((0.3, 0.2, 0.1), (2.5, 2.8, 3.0), 0.4)
        s.add_triangle_mesh(scenes._aabb((-2.45, 0.01, -2.45), (2.45, 2.3, 2.45)), 0, interior=fog, exterior=0)
        s.add_triangle_mesh(scenes._aabb((-1.3, 0.5, -0.5), (-0.6, 1.3, 0.2)), 0, interior=dense, exterior=fog)
    if emitter == "quad":
        al = s.add_area_light_diffuse((9.0, 8.0, 6.0))
        s.add_triangle_mesh(_quad([[-.5, 2.2, -.5], [.5, 2.2, -.5], [.5, 2.2, .5], [-.5, 2.2, .5]]), s.add_matte((0, 0, 0)),
                            area_light=al, interior=fog, exterior=fog)
    elif emitter == "mesh":  # (displaced_sphere winds its triangles inwards, and a triangle emits on its front side only)
        ball = scenes.displaced_sphere(40, 44, radius=0.45, amplitude=0.1, seed=9)
        ball.indices = np.ascontiguousarray(ball.indices.reshape(-1, 3)[:, ::-1].reshape(-1))
        al = s.add_area_light_diffuse((3.0, 2.6, 2.0))
        s.add_triangle_mesh(ball, s.add_matte((0, 0, 0)), area_light=al, ctm=glam.from_translation((-0.4, 1.5, 0.6)))
    if sun:
        s.add_light_distant((1.0, 2.0, -1.5), (0.0, 0.0, 0.0), (2.5, 2.4, 2.2))
    if sky:
        s.set_infinite_light((0.3, 0.35, 0.45))
    return s


def _cornell_sun():
    s = scenes.cornell_box(W, H)
    s.add_light_distant((-0.18862, 0.692312, 0.69651), (0, 0, 0), (8, 8, 8))  # dragon/scene.pbrt:44
    return s


class Entry(NamedTuple):
    name: str
    family: str   # "item", "restart", "vol-item", "vol-restart" (VARIANTS)
    leaf: int     # FEAT of the kernel the family's default dispatch picks
    cls: str      # tolerance class (TOL)
    build: Callable[[], Scene]


CATALOGUE = (
    # path integrator, wave-coherent item loop
    Entry("cornell", "item", 64, "matte", lambda: scenes.cornell_box(W, H)),
    Entry("cornell+sun", "item", 72, "matte", _cornell_sun),
    Entry("metal", "item", 835, "single", lambda: room(["metal"])),
    Entry("metal+spheres", "item", 835, "single", lambda: room(["metal"], spheres=True)),
    Entry("glass-mirror+spheres", "item", 67, "multi", lambda: room(["glass", "mirror"], spheres=True)),
    Entry("metal+spheres+sun", "item", 95, "single", lambda: room(["metal"], spheres=True, sun=True)),
    Entry("glass-mirror+sun", "item", 95, "multi", lambda: room(["glass", "mirror"], sun=True)),
    Entry("plastic-uber", "item", 127, "multi", lambda: room(["plastic", "uber"], spheres=True, sun=True, sky=True, textures=True)),
    # path integrator, BVH deeper than 512 nodes: traversal restart (and, under NO_RESTART, the while-while kernel)
    Entry("matte-deep+emitter", "restart", 8, "matte", lambda: room(deep="matte")),
    Entry("matte+emissive-mesh", "restart", 8, "matte", lambda: room(emitter="mesh")),
    Entry("matte-deep+sun", "restart", 2056, "matte", lambda: room(deep="matte", emitter=None, sun=True)),
    Entry("substrate-deep+emitter", "restart", 1302, "single", lambda: room(deep="substrate", textures=True, sky=True)),
    Entry("substrate-deep+sky", "restart", 3350, "single", lambda: room(deep="substrate", emitter=None, textures=True, sky=True)),
    Entry("metal-deep", "restart", 22, "single", lambda: room(deep="metal")),
    Entry("glass-deep+mirror", "restart", 22, "multi", lambda: room(["mirror"], deep="glass")),
    Entry("metal-deep+spheres+sun", "restart", 31, "single", lambda: room(["metal"], spheres=True, deep="metal", sun=True)),
    Entry("glass-deep+mirror+sun", "restart", 31, "multi", lambda: room(["mirror"], deep="glass", sun=True)),
    Entry("plastic-uber-deep", "restart", 63, "multi",
          lambda: room(["plastic", "uber"], spheres=True, deep="uber", sun=True, sky=True, textures=True)),
    # volumetric integrator: media behind None-material boundaries
    Entry("fog", "vol-item", 200, "vol", lambda: room(volpath=True, sun=True)),
    Entry("fog+glass", "vol-item", 223, "multi", lambda: room(["glass"], spheres=True, volpath=True)),
    Entry("fog+plastic", "vol-item", 255, "multi", lambda: room(["plastic"], volpath=True, sun=True)),
    Entry("fog-deep", "vol-restart", 136, "vol", lambda: room(deep="matte", volpath=True, sun=True)),
    Entry("fog-deep+substrate+glass", "vol-restart", 159, "multi", lambda: room(["glass"], deep="substrate", volpath=True)),
    Entry("fog-deep+uber", "vol-restart", 191, "multi", lambda: room(["plastic"], spheres=True, deep="uber", volpath=True, sun=True)),
)
BY_NAME = {e.name: e for e in CATALOGUE}
