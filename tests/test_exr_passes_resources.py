"""CPU: what the compiler reports for the pass-layer pack's gfx950 kernel (rene_amd/csrc/kernels_exr_passes.res, written by the Makefile with
`-Rpass-analysis=kernel-resource-usage`): ONE kernel for every combination of layers and groups, no scratch, no LDS, no spill.  The design's
choice is pinned: the loads are grouped per source record, each group ahead of its own conversions, so the widest group -- the bounce record's
ten sums and its counts -- sets the registers, not all 104 dwords of the four records at once.  The registers and waves are the ones the compiler
gave when the kernel was written."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "rene_amd", "csrc")
RES = os.path.join(CSRC, "kernels_exr_passes.res")
VGPRS, WAVES = 44, 8


def test_one_kernel_its_registers_and_no_scratch(hip_lib):
    text = open(RES).read()
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 1 and re.fullmatch(r"_ZN4rene\d+exr_passes_kernelENS_15ExrPassesLaunchE", names[0]), names
    g = lambda key: int(re.search(re.escape(key) + r": (\d+)", text).group(1))
    assert g("ScratchSize [bytes/lane]") == 0 and g("LDS Size [bytes/block]") == 0 and g("SGPRs Spill") == 0 and g("VGPRs Spill") == 0
    assert (g("VGPRs"), g("Occupancy [waves/SIMD]")) == (VGPRS, WAVES)
    assert g("VGPRs") < 64  # well below the 104 dwords of the four records: the groups do not overlap
