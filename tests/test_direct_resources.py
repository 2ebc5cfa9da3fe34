"""CPU: what the compiler reports for the direct-light pass's gfx950 kernels (rene_amd/csrc/kernels_direct.res, written by the Makefile with
`-Rpass-analysis=kernel-resource-usage`): direct_kernel and direct_samples_kernel, each for the item loop (SMALL) and for the BVH, each with the
Matte-only BSDF and with the general five-lobe one.  Nothing else is in the unit, none has static LDS (the BVH instantiations' traversal stack
is dynamic, sized at the launch), none combines SGPR and VGPR spills, the Matte instantiations are scratch-free, the five-lobe ones need the 64
bytes per lane DESIGN.md states, and the registers are the ones the compiler gave when the kernels were written."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "rene_amd", "csrc")
RES = os.path.join(CSRC, "kernels_direct.res")
# (kernel, SMALL, MATTE) -> VGPRs, waves per SIMD, scratch bytes per lane
PINNED = {("direct_kernel", 1, 1): (79, 6, 0), ("direct_kernel", 0, 1): (111, 4, 0), ("direct_kernel", 1, 0): (181, 2, 64),
          ("direct_kernel", 0, 0): (195, 2, 64), ("direct_samples_kernel", 1, 1): (81, 5, 0), ("direct_samples_kernel", 0, 1): (107, 4, 0),
          ("direct_samples_kernel", 1, 0): (177, 2, 64), ("direct_samples_kernel", 0, 0): (191, 2, 64)}


def _kernels():
    text = open(RES).read()
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", text, re.S):
        g = lambda key: int(re.search(re.escape(key) + r": (\d+)", m.group(2)).group(1))
        out[m.group(1)] = {"vgpr": g("VGPRs"), "scratch": g("ScratchSize [bytes/lane]"), "occupancy": g("Occupancy [waves/SIMD]"),
                           "sgpr_spill": g("SGPRs Spill"), "vgpr_spill": g("VGPRs Spill"), "lds": int(m.group(3))}
    return out


def test_the_catalogue_its_scratch_spills_and_static_lds(hip_lib):
    ks = _kernels()
    names = {}
    for n in ks:
        m = re.fullmatch(r"_ZN4rene\d+(direct_kernel|direct_samples_kernel)ILb([01])ELb([01])EEEvNS_9SceneViewENS_12DirectLaunchE", n)
        assert m, n  # nothing else is instantiated in this unit: no render kernel, no probe of device_code.inc
        names[m.group(1), int(m.group(2)), int(m.group(3))] = ks[n]
    assert set(names) == set(PINNED) and len(ks) == 8, list(ks)
    for key, k in names.items():
        assert k["lds"] == 0, (key, k)
        assert not (k["sgpr_spill"] and k["vgpr_spill"]), (key, k)  # the project's miscompile rule (tests/test_kernel_resources.py)
        assert k["vgpr_spill"] == 0, (key, k)  # (and as written no vector register is spilled)
        if key[2]:
            assert k["scratch"] == 0, (key, k)  # the Matte instantiations are scratch-free
        assert (k["vgpr"], k["occupancy"], k["scratch"]) == PINNED[key], (key, k)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "kernels_direct.hip" in design and "64 bytes of scratch" in design  # the figure is stated, not hidden


def test_the_unit_is_in_the_makefile_with_the_render_kernels_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    assert "kernels_direct.o" in objs
    rule = re.search(r"^kernels_direct\.o: kernels_direct\.hip primary_ray\.h \$\(HDRS\)\n\t(.*)$", mk, re.M).group(1)
    assert "$(HIPFLAGS)" in rule and "$(ROBUSTFLAGS)" not in rule and "$(RESFLAGS)" in rule and "2> kernels_direct.res" in rule
    variant = mk[mk.index("\nvariant:"):mk.index("\nclean:")]
    assert "$(HIPFLAGS) $(RESFLAGS) $(EXTRA) -c -o var_$(NAME)/kernels_direct.o kernels_direct.hip" in variant
    # the unit includes what the geometry pass includes (pixel_pass.h behind them: what the per-pixel passes share), and no other unit knows of it
    src = open(os.path.join(CSRC, "kernels_direct.hip")).read()
    assert '#include "primary_ray.h"' in src and '#include "device_code.inc"' in src
    assert not re.search(r"atomic[A-Z_(]", src)  # the sums stay in registers
    for unit in os.listdir(CSRC):
        if unit.endswith((".hip", ".inc")) and unit != "kernels_direct.hip":
            assert "direct_kernel" not in open(os.path.join(CSRC, unit)).read() and "launch_direct" not in open(os.path.join(CSRC, unit)).read(), unit
