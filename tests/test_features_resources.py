"""CPU: what the compiler reports for the feature export's gfx950 kernels (rene_amd/csrc/kernels_features.res, written by the Makefile with
`-Rpass-analysis=kernel-resource-usage`): four instantiations (fp32 / fp16 x planar / interleaved), none with scratch or spills, the registers
and occupancy that were measured when the kernel was written, and LDS only where the interleaved layout stages its rows."""
import os
import re

from conftest import ROOT

RES = os.path.join(ROOT, "rene_amd", "csrc", "kernels_features.res")
# (element, interleaved): VGPRs, waves per SIMD, LDS bytes as measured (hipcc of ROCm 7, gfx950).  The interleaved kernels stage 8 rows x 32 pixels x
# 17 channels of their element; a workgroup is one wave per SIMD, so an occupancy of 5 is five workgroups per compute unit: 85 KB of the 160 KB LDS
MEASURED = {("f", True): (96, 5, 256 * 17 * 4), ("f", False): (70, 7, 0), ("DF16_", True): (88, 5, 256 * 17 * 2), ("DF16_", False): (73, 6, 0)}


def _kernels():
    text = open(RES).read()
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", text, re.S):
        g = lambda key: int(re.search(re.escape(key) + r": (\d+)", m.group(2)).group(1))
        out[m.group(1)] = {"vgpr": g("VGPRs"), "scratch": g("ScratchSize [bytes/lane]"), "occupancy": g("Occupancy [waves/SIMD]"),
                           "sgpr_spill": g("SGPRs Spill"), "vgpr_spill": g("VGPRs Spill"), "lds": int(m.group(3))}
    return out


def test_every_instantiation_is_there_without_scratch_or_spills(hip_lib):
    ks = _kernels()
    assert len(ks) == 4 and all("features_kernel" in name for name in ks), list(ks)
    seen = set()
    for name, k in ks.items():
        m = re.search(r"features_kernelI(f|DF16_)Lb([01])E", name)  # the mangled template arguments: element type, interleaved
        assert m, name
        key = (m.group(1), m.group(2) == "1")
        seen.add(key)
        vgpr, occupancy, lds = MEASURED[key]
        assert k["scratch"] == 0 and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0, (name, k)
        assert k["vgpr"] <= vgpr and k["occupancy"] >= occupancy, (name, k)  # no worse than measured
        assert k["lds"] == lds, (name, k)
    assert seen == set(MEASURED)
