"""CPU: what the compiler reports for the output transform's gfx950 kernels (rene_amd/csrc/kernels_output.res, written by the Makefile with
`-Rpass-analysis=kernel-resource-usage`): transform x format instantiations of the image kernel and one probe per transform, none with scratch
or spills, the threshold table the only LDS (under 2 KB, and only in the sRGB instantiations), at least four waves per SIMD."""
import os
import re

from conftest import ROOT

RES = os.path.join(ROOT, "rene_amd", "csrc", "kernels_output.res")


def _kernels():
    text = open(RES).read()
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", text, re.S):
        g = lambda key: int(re.search(re.escape(key) + r": (\d+)", m.group(2)).group(1))
        out[m.group(1)] = {"vgpr": g("VGPRs"), "scratch": g("ScratchSize [bytes/lane]"), "occupancy": g("Occupancy [waves/SIMD]"),
                           "sgpr_spill": g("SGPRs Spill"), "vgpr_spill": g("VGPRs Spill"), "lds": int(m.group(3))}
    return out


def test_every_kernel_is_there_without_scratch_or_spills(hip_lib):
    ks = _kernels()
    image = {re.search(r"output_kernelILi(\d)ELi(\d)EE", n).groups() for n in ks if "output_kernel" in n}
    probe = {re.search(r"output_probe_kernelILi(\d)EE", n).group(1) for n in ks if "output_probe_kernel" in n}
    assert image == {(t, f) for t in "012" for f in "01"} and probe == set("012") and len(ks) == 9, list(ks)
    for name, k in ks.items():
        assert k["scratch"] == 0 and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0, (name, k)
        assert k["lds"] < 2048 and k["occupancy"] >= 4, (name, k)
        srgb = "ILi0E" in name
        assert k["lds"] == (1024 if srgb else 0), (name, k)  # the 255 thresholds, padded to 256 floats
