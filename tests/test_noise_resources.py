"""CPU: what the compiler reports for the noise estimate's gfx950 kernel (rene_amd/csrc/kernels_noise.res, written by the Makefile with
`-Rpass-analysis=kernel-resource-usage`): no scratch, no spills, and an LDS footprint of the four wave partials only."""
import os
import re

from conftest import ROOT

RES = os.path.join(ROOT, "rene_amd", "csrc", "kernels_noise.res")


def _kernels():
    text = open(RES).read()
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", text, re.S):
        g = lambda key: int(re.search(re.escape(key) + r": (\d+)", m.group(2)).group(1))
        out[m.group(1)] = {"vgpr": g("VGPRs"), "scratch": g("ScratchSize [bytes/lane]"), "occupancy": g("Occupancy [waves/SIMD]"),
                           "sgpr_spill": g("SGPRs Spill"), "vgpr_spill": g("VGPRs Spill"), "lds": int(m.group(3))}
    return out


def test_noise_kernel_has_no_scratch_no_spills_and_little_lds(hip_lib):
    ks = _kernels()
    assert len(ks) == 1 and "noise_tiles_kernel" in next(iter(ks)), ks
    (k,) = ks.values()
    assert k["scratch"] == 0 and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0, k
    assert 0 < k["lds"] <= 256, k       # three words per wave, four waves
    assert k["vgpr"] >= 128, k          # the 32 16-byte records a thread loads before it uses any are held in registers ...
    assert k["occupancy"] >= 2, k       # ... and still more than one workgroup fits a compute unit (a workgroup is one wave per SIMD)


def test_unit_is_in_the_makefile():
    mk = open(os.path.join(ROOT, "rene_amd", "csrc", "Makefile")).read()
    assert "kernels_noise.o" in mk.split("OBJS =")[1].splitlines()[0]
    assert "2> kernels_noise.res" in mk
    assert "kernels_noise" in [l for l in mk.splitlines() if l.lstrip().startswith("for u in kernels ")][0]
