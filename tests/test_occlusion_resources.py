"""CPU: what the compiler reports for the occlusion pass's gfx950 kernels (rene_amd/csrc/kernels_occlusion.res, written by the Makefile with
`-Rpass-analysis=kernel-resource-usage`): occlusion_kernel and occlusion_samples_kernel, each for the item loop (SMALL) and for the BVH, none with
scratch, none that combines SGPR and VGPR spills, no static LDS (the BVH instantiations' traversal stack is dynamic, sized at the launch), and
the registers the compiler gave when the kernels were written."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "rene_amd", "csrc")
RES = os.path.join(CSRC, "kernels_occlusion.res")
# (kernel, SMALL) -> VGPRs, waves per SIMD
PINNED = {("occlusion_kernel", 1): (51, 8), ("occlusion_kernel", 0): (86, 5), ("occlusion_samples_kernel", 1): (60, 7),
          ("occlusion_samples_kernel", 0): (86, 5)}


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
        m = re.fullmatch(r"_ZN4rene\d+(occlusion_kernel|occlusion_samples_kernel)ILb([01])EEEvNS_9SceneViewENS_15OcclusionLaunchE", n)
        assert m, n  # nothing else is instantiated in this unit: no render kernel, no probe of device_code.inc
        names[m.group(1), int(m.group(2))] = ks[n]
    assert set(names) == set(PINNED) and len(ks) == 4, list(ks)
    for key, k in names.items():
        assert k["scratch"] == 0 and k["lds"] == 0, (key, k)
        assert not (k["sgpr_spill"] and k["vgpr_spill"]), (key, k)  # the project's miscompile rule (tests/test_kernel_resources.py)
        assert k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0, (key, k)  # (and as written there is neither)
        assert (k["vgpr"], k["occupancy"]) == PINNED[key], (key, k)


def test_the_unit_is_in_the_makefile_with_the_render_kernels_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    assert "kernels_occlusion.o" in objs
    rule = re.search(r"^kernels_occlusion\.o: kernels_occlusion\.hip primary_ray\.h \$\(HDRS\)\n\t(.*)$", mk, re.M).group(1)
    assert "$(HIPFLAGS)" in rule and "$(ROBUSTFLAGS)" not in rule and "$(RESFLAGS)" in rule and "2> kernels_occlusion.res" in rule
    variant = mk[mk.index("\nvariant:"):mk.index("\nclean:")]
    assert "$(HIPFLAGS) $(RESFLAGS) $(EXTRA) -c -o var_$(NAME)/kernels_occlusion.o kernels_occlusion.hip" in variant
    # the unit includes what the geometry pass includes (pixel_pass.h behind them: what the per-pixel passes share), and the geometry pass's unit
    # does not know of it
    src = open(os.path.join(CSRC, "kernels_occlusion.hip")).read()
    assert '#include "primary_ray.h"' in src and '#include "device_code.inc"' in src
    assert not re.search(r"atomic[A-Z_(]", src)  # counts and sums stay in registers
    assert "occlusion" not in open(os.path.join(CSRC, "kernels_gbuffer.hip")).read()
