"""CPU: what the compiler reports for the geometry pass's gfx950 kernels (rene_amd/csrc/kernels_gbuffer.res, written by the Makefile with
`-Rpass-analysis=kernel-resource-usage`): gbuffer_kernel and primary_hits_kernel, each for the item loop (SMALL) and for the BVH, none with scratch
or spills, no static LDS (the BVH instantiations' traversal stack is dynamic, sized at the launch), and the registers the compiler gave when the
kernels were written."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "rene_amd", "csrc")
RES = os.path.join(CSRC, "kernels_gbuffer.res")
# (kernel, SMALL) -> VGPRs, waves per SIMD
PINNED = {("gbuffer_kernel", 1): (46, 8), ("gbuffer_kernel", 0): (78, 6), ("primary_hits_kernel", 1): (36, 8), ("primary_hits_kernel", 0): (68, 7)}


def _kernels():
    text = open(RES).read()
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", text, re.S):
        g = lambda key: int(re.search(re.escape(key) + r": (\d+)", m.group(2)).group(1))
        out[m.group(1)] = {"vgpr": g("VGPRs"), "scratch": g("ScratchSize [bytes/lane]"), "occupancy": g("Occupancy [waves/SIMD]"),
                           "sgpr_spill": g("SGPRs Spill"), "vgpr_spill": g("VGPRs Spill"), "lds": int(m.group(3))}
    return out


def test_the_catalogue_without_scratch_spills_or_static_lds(hip_lib):
    ks = _kernels()
    names = {}
    for n in ks:
        m = re.fullmatch(r"_ZN4rene\d+(gbuffer_kernel|primary_hits_kernel)ILb([01])EEEvNS_9SceneViewENS_13GbufferLaunchE", n)
        assert m, n  # nothing else is instantiated in this unit: no render kernel, no probe of device_code.inc
        names[m.group(1), int(m.group(2))] = ks[n]
    assert set(names) == set(PINNED) and len(ks) == 4, list(ks)
    for key, k in names.items():
        assert k["scratch"] == 0 and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0 and k["lds"] == 0, (key, k)
        assert (k["vgpr"], k["occupancy"]) == PINNED[key], (key, k)


def test_the_unit_is_in_the_makefile_with_the_render_kernels_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    assert "kernels_gbuffer.o" in objs
    rule = re.search(r"^kernels_gbuffer\.o: kernels_gbuffer\.hip primary_ray\.h \$\(HDRS\)\n\t(.*)$", mk, re.M).group(1)
    assert "$(HIPFLAGS)" in rule and "$(ROBUSTFLAGS)" not in rule and "$(RESFLAGS)" in rule and "2> kernels_gbuffer.res" in rule
    variant = mk[mk.index("\nvariant:"):mk.index("\nclean:")]
    assert "var_$(NAME)/kernels_gbuffer.o kernels_gbuffer.hip" in variant
    # the render kernels do not call the new header: their text is what it was
    for unit in ("device_code.inc", "render_wf.inc", "wavefront.inc", "kernels.hip", "kernels_bvh.hip", "kernels_vol.hip", "kernels_wave.hip"):
        assert "primary_ray" not in open(os.path.join(CSRC, unit)).read(), unit
