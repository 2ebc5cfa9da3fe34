"""CPU: what the compiler reports for the gfx950 kernels of the denoiser's tile-by-tile unit (rene_amd/csrc/kernels_denoise_tiles.res, written by
the Makefile with `-Rpass-analysis=kernel-resource-usage`): no scratch, no spills, and the LDS-staged masked passes with the LDS and the room for
two workgroups per compute unit that tests/test_denoise_resources.py asks of the unmasked ones."""
import os
import re

from conftest import ROOT

RES = os.path.join(ROOT, "rene_amd", "csrc", "kernels_denoise_tiles.res")
LDS_PER_CU = 160 * 1024


def _kernels():
    text = open(RES).read()
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", text, re.S):
        g = lambda key: int(re.search(re.escape(key) + r": (\d+)", m.group(2)).group(1))
        out[m.group(1)] = {"sgpr": g("TotalSGPRs"), "vgpr": g("VGPRs"), "scratch": g("ScratchSize [bytes/lane]"),
                           "occupancy": g("Occupancy [waves/SIMD]"), "sgpr_spill": g("SGPRs Spill"), "vgpr_spill": g("VGPRs Spill"),
                           "lds": int(m.group(3))}
    return out


def test_tile_kernels_have_no_scratch_and_no_spills(hip_lib):
    ks = _kernels()
    names = " ".join(ks)
    for kernel in ("denoise_tiles_prepare_kernel", "denoise_tiles_finalize_kernel", "denoise_mean_kernel"):
        assert kernel in names, kernel
    for s in (0, 1, 2, 4):  # the direct masked pass and the three staged ones
        assert f"atrous_pass_tiles_kernelILi{s}E" in names, s
    assert len(ks) == 7
    for name, k in ks.items():
        assert k["scratch"] == 0 and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0, (name, k)


def test_staged_masked_passes_leave_room_for_two_workgroups_per_cu(hip_lib):
    ks = _kernels()
    staged = {n: k for n, k in ks.items() if "atrous_pass_tiles_kernel" in n and "ILi0E" not in n}
    assert len(staged) == 3
    for name, k in staged.items():
        assert 0 < k["lds"] <= 80 * 1024 and 2 * k["lds"] <= LDS_PER_CU, (name, k)
        assert k["occupancy"] >= 2, (name, k)  # a workgroup is four waves, one per SIMD: two workgroups per CU = two waves per SIMD
    direct = [k for n, k in ks.items() if "atrous_pass_tiles_kernelILi0E" in n]
    assert len(direct) == 1 and direct[0]["lds"] == 0
    # 32 x 8 tile + halo of 2 s, three 16-byte records per pixel: the mask travels in the records, the layout is the unmasked passes'
    for s in (1, 2, 4):
        (k,) = [k for n, k in staged.items() if f"ILi{s}E" in n]
        assert k["lds"] == (32 + 4 * s) * (8 + 4 * s) * 48, (s, k)
