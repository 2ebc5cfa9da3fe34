"""CPU: what the compiler reports for the light-group pass's gfx950 kernels (rene_amd/csrc/kernels_lights.res, written by the Makefile with
`-Rpass-analysis=kernel-resource-usage`): lights_kernel and lights_samples_kernel, each for the item loop (SMALL) and for the BVH, each with the
Matte-only BSDF and with the general five-lobe one.  Nothing else is in the unit; no vector register is spilled and none combines SGPR and VGPR
spills; the Matte instantiations are scratch-free and the five-lobe ones need no more than the bounce pass's 64 bytes per lane.  The design's
choice is pinned: ONE static LDS column per lane, the sample's 32 group words (32 x 256 x 4 bytes), in the pass's kernels and in the probe's --
the pixel's 32 words are registers, not a second column (which would read 65 536 here) -- and the registers and waves are the ones the compiler
gave when the kernels were written, which DESIGN.md states."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "rene_amd", "csrc")
RES = os.path.join(CSRC, "kernels_lights.res")
LDS = 32 * 256 * 4
# (kernel, SMALL, MATTE) -> VGPRs, waves per SIMD, scratch bytes per lane, static LDS bytes per workgroup
PINNED = {("lights_kernel", 1, 1): (113, 4, 0, LDS), ("lights_kernel", 0, 1): (129, 3, 0, LDS), ("lights_kernel", 1, 0): (219, 2, 64, LDS),
          ("lights_kernel", 0, 0): (233, 2, 64, LDS), ("lights_samples_kernel", 1, 1): (93, 5, 0, LDS), ("lights_samples_kernel", 0, 1): (119, 4, 0, LDS),
          ("lights_samples_kernel", 1, 0): (193, 2, 64, LDS), ("lights_samples_kernel", 0, 0): (207, 2, 64, LDS)}


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
        m = re.fullmatch(r"_ZN4rene\d+(lights_kernel|lights_samples_kernel)ILb([01])ELb([01])EEEvNS_9SceneViewENS_12LightsLaunchE", n)
        assert m, n  # nothing else is instantiated in this unit: no render kernel, no probe of device_code.inc
        names[m.group(1), int(m.group(2)), int(m.group(3))] = ks[n]
    assert set(names) == set(PINNED) and len(ks) == 8, list(ks)
    for key, k in names.items():
        assert k["vgpr_spill"] == 0, (key, k)  # no vector register is spilled
        assert not (k["sgpr_spill"] and k["vgpr_spill"]), (key, k)  # the project's miscompile rule (tests/test_kernel_resources.py)
        if key[2]:
            assert k["scratch"] == 0, (key, k)  # the Matte instantiations are scratch-free
        assert k["scratch"] <= 64, (key, k)  # the general form: no more than the bounce pass's
        assert k["lds"] == LDS, (key, k)  # the sample's column and nothing else: the pixel's sums are registers
        assert (k["vgpr"], k["occupancy"], k["scratch"], k["lds"]) == PINNED[key], (key, k)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "kernels_lights.hip" in design and "32 768 bytes" in design and "65 536" in design  # the choice and what it was weighed against are stated
    section = design[design.index("kernels_lights.hip"):]
    for key, (vgpr, occupancy, _, _) in PINNED.items():
        assert f"{vgpr} / {occupancy}" in section, (key, vgpr, occupancy)


def test_the_unit_is_in_the_makefile_with_the_render_kernels_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", mk, re.M).group(1).split()
    assert "kernels_lights.o" in objs
    rule = re.search(r"^kernels_lights\.o: kernels_lights\.hip primary_ray\.h \$\(HDRS\)\n\t(.*)$", mk, re.M).group(1)
    assert "$(HIPFLAGS)" in rule and "$(ROBUSTFLAGS)" not in rule and "$(RESFLAGS)" in rule and "2> kernels_lights.res" in rule
    assert re.search(r"^kernels_lights\.o: pixel_pass\.h$", mk, re.M)  # a dependency line of its own
    assert re.search(r"^kernels_gbuffer\.o kernels_occlusion\.o kernels_direct\.o kernels_bounces\.o: pixel_pass\.h$", mk, re.M)  # (the four's, as it was)
    variant = mk[mk.index("\nvariant:"):mk.index("\nclean:")]
    assert "$(HIPFLAGS) $(RESFLAGS) $(EXTRA) -c -o var_$(NAME)/kernels_lights.o kernels_lights.hip" in variant
    src = open(os.path.join(CSRC, "kernels_lights.hip")).read()
    assert '#include "primary_ray.h"' in src and '#include "device_code.inc"' in src and '#include "pixel_pass.h"' in src
    assert "atomic" not in src  # the sums stay on chip, a lane to itself
    for theirs in ("bounces_kernel", "launch_bounces", "direct_kernel", "launch_direct"):
        assert theirs not in src, theirs  # (tests/test_bounces_resources.py, tests/test_direct_resources.py: no other unit names them)
    for unit in os.listdir(CSRC):
        if unit.endswith((".hip", ".inc")) and unit != "kernels_lights.hip":
            text = open(os.path.join(CSRC, unit)).read()
            assert "lights_kernel" not in text and "launch_lights" not in text and "lights_samples_kernel" not in text, unit
