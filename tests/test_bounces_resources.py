"""CPU: what the compiler reports for the bounce pass's gfx950 kernels (rene_amd/csrc/kernels_bounces.res, written by the Makefile with
`-Rpass-analysis=kernel-resource-usage`): bounces_kernel and bounces_samples_kernel, each for the item loop (SMALL) and for the BVH, each with the
Matte-only BSDF and with the general five-lobe one.  Nothing else is in the unit; no vector register is spilled and none combines SGPR and VGPR
spills; the Matte instantiations are scratch-free and the five-lobe ones need no more than the direct-light pass's 64 bytes per lane; the pass's
kernels hold the pixel's 40 bucket words in a static LDS column per lane (40 x 256 x 4 bytes) and the probe's hold none (the BVH instantiations'
traversal stack is dynamic, sized at the launch); the registers are the ones the compiler gave when the kernels were written, and DESIGN.md
states them."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "rene_amd", "csrc")
RES = os.path.join(CSRC, "kernels_bounces.res")
LDS = 40 * 256 * 4
# (kernel, SMALL, MATTE) -> VGPRs, waves per SIMD, scratch bytes per lane, static LDS bytes per workgroup
PINNED = {("bounces_kernel", 1, 1): (93, 4, 0, LDS), ("bounces_kernel", 0, 1): (121, 4, 0, LDS), ("bounces_kernel", 1, 0): (200, 2, 64, LDS),
          ("bounces_kernel", 0, 0): (213, 2, 64, LDS), ("bounces_samples_kernel", 1, 1): (102, 4, 0, 0), ("bounces_samples_kernel", 0, 1): (129, 3, 0, 0),
          ("bounces_samples_kernel", 1, 0): (203, 2, 64, 0), ("bounces_samples_kernel", 0, 0): (217, 2, 64, 0)}


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
        m = re.fullmatch(r"_ZN4rene\d+(bounces_kernel|bounces_samples_kernel)ILb([01])ELb([01])EEEvNS_9SceneViewENS_13BouncesLaunchE", n)
        assert m, n  # nothing else is instantiated in this unit: no render kernel, no probe of device_code.inc
        names[m.group(1), int(m.group(2)), int(m.group(3))] = ks[n]
    assert set(names) == set(PINNED) and len(ks) == 8, list(ks)
    for key, k in names.items():
        assert k["vgpr_spill"] == 0, (key, k)  # no vector register is spilled
        assert not (k["sgpr_spill"] and k["vgpr_spill"]), (key, k)  # the project's miscompile rule (tests/test_kernel_resources.py)
        if key[2]:
            assert k["scratch"] == 0, (key, k)  # the Matte instantiations are scratch-free
        assert k["scratch"] <= 64, (key, k)  # the general form: no more than the direct-light pass's
        assert k["lds"] == (LDS if key[0] == "bounces_kernel" else 0), (key, k)
        assert (k["vgpr"], k["occupancy"], k["scratch"], k["lds"]) == PINNED[key], (key, k)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "kernels_bounces.hip" in design and "40 960 bytes" in design and "64 bytes of scratch" in design  # the figures are stated, not hidden
    section = design[design.index("kernels_bounces.hip"):]
    for key, (vgpr, occupancy, _, _) in PINNED.items():
        assert f"{vgpr} / {occupancy}" in section, (key, vgpr, occupancy)


def test_the_unit_is_in_the_makefile_with_the_render_kernels_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    assert "kernels_bounces.o" in objs
    rule = re.search(r"^kernels_bounces\.o: kernels_bounces\.hip primary_ray\.h \$\(HDRS\)\n\t(.*)$", mk, re.M).group(1)
    assert "$(HIPFLAGS)" in rule and "$(ROBUSTFLAGS)" not in rule and "$(RESFLAGS)" in rule and "2> kernels_bounces.res" in rule
    assert re.search(r"^kernels_gbuffer\.o .*kernels_bounces\.o: pixel_pass\.h$", mk, re.M)
    variant = mk[mk.index("\nvariant:"):mk.index("\nclean:")]
    assert "$(HIPFLAGS) $(RESFLAGS) $(EXTRA) -c -o var_$(NAME)/kernels_bounces.o kernels_bounces.hip" in variant
    src = open(os.path.join(CSRC, "kernels_bounces.hip")).read()
    assert '#include "primary_ray.h"' in src and '#include "device_code.inc"' in src and '#include "pixel_pass.h"' in src
    assert "atomic" not in src  # the sums stay on chip, a lane to itself
    assert "direct_kernel" not in src and "launch_direct" not in src  # (tests/test_direct_resources.py: no other unit names them)
    for unit in os.listdir(CSRC):
        if unit.endswith((".hip", ".inc")) and unit != "kernels_bounces.hip":
            text = open(os.path.join(CSRC, unit)).read()
            assert "bounces_kernel" not in text and "launch_bounces" not in text, unit
