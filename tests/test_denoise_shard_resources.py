"""CPU: what the compiler reports for the gfx950 kernels of the denoiser's tile-shard unit (rene_amd/csrc/kernels_denoise_shard.res, written by the
Makefile with `-Rpass-analysis=kernel-resource-usage`): the packed prepare and the place kernel, both without scratch, spills or LDS.  The unit is
one of its own, so the kernel counts tests/test_denoise_resources.py and tests/test_denoise_tiles_resources.py pin stay what they are.

That the kernels of those two units are instruction for instruction what they were is checked by hand, not here: compile kernels_denoise.hip and
kernels_denoise_tiles.hip with the Makefile's HIPFLAGS and `--cuda-device-only -S` at the parent commit and at this one and diff the two listings
-- they differ in the compilation-unit id (`__hip_cuid_...`) alone, because with ATROUS_PACKED off the preprocessor leaves atrous_kernels.inc's
text for them as it was."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "rene_amd", "csrc")
RES = os.path.join(CSRC, "kernels_denoise_shard.res")


def _kernels():
    text = open(RES).read()
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", text, re.S):
        g = lambda key: int(re.search(re.escape(key) + r": (\d+)", m.group(2)).group(1))
        out[m.group(1)] = {"sgpr": g("TotalSGPRs"), "vgpr": g("VGPRs"), "scratch": g("ScratchSize [bytes/lane]"),
                           "occupancy": g("Occupancy [waves/SIMD]"), "sgpr_spill": g("SGPRs Spill"), "vgpr_spill": g("VGPRs Spill"),
                           "lds": int(m.group(3))}
    return out


def test_shard_kernels_have_no_scratch_no_spills_and_no_lds(hip_lib):
    ks = _kernels()
    names = " ".join(ks)
    for kernel in ("denoise_shard_prepare_kernel", "denoise_shard_place_kernel"):
        assert kernel in names, kernel
    assert len(ks) == 2  # the pass text of atrous_kernels.inc is not compiled into this unit
    for name, k in ks.items():
        assert k["scratch"] == 0 and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0 and k["lds"] == 0, (name, k)
        assert k["occupancy"] >= 4, (name, k)  # streaming kernels: registers must not be what limits the waves in flight

