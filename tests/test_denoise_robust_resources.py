"""CPU: what the compiler reports for the gfx950 kernels of the denoiser's trimmed prepare (rene_amd/csrc/kernels_denoise_robust.res and
kernels_denoise_trim.res, written by the Makefile with `-Rpass-analysis=kernel-resource-usage`): exactly the new kernels, no scratch, no spills,
no LDS -- and the two existing units of the denoiser still hold the kernels they held."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "rene_amd", "csrc")


def _kernels(unit):
    text = open(os.path.join(CSRC, unit + ".res")).read()
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", text, re.S):
        g = lambda key: int(re.search(re.escape(key) + r": (\d+)", m.group(2)).group(1))
        out[m.group(1)] = {"vgpr": g("VGPRs"), "scratch": g("ScratchSize [bytes/lane]"), "occupancy": g("Occupancy [waves/SIMD]"),
                           "sgpr_spill": g("SGPRs Spill"), "vgpr_spill": g("VGPRs Spill"), "lds": int(m.group(3))}
    return out


def _only(ks, *names):
    assert len(ks) == len(names), sorted(ks)
    for n in names:
        assert sum(re.search(r"\d" + n + "E", k) is not None for k in ks) == 1, (n, sorted(ks))  # the mangled name: <length><name>E


def test_the_new_units_hold_exactly_the_new_kernels(hip_lib):
    prepare, trim = _kernels("kernels_denoise_robust"), _kernels("kernels_denoise_trim")
    _only(prepare, "denoise_robust_prepare_kernel", "denoise_tiles_robust_prepare_kernel")
    _only(trim, "denoise_trim_kernel")
    for name, k in {**prepare, **trim}.items():
        assert k["scratch"] == 0 and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0 and k["lds"] == 0, (name, k)
        assert k["vgpr"] <= 64 and k["occupancy"] >= 8, (name, k)  # eight float4 records in flight and room for every wave a SIMD can hold


def test_the_existing_units_are_what_they_were(hip_lib):
    assert len(_kernels("kernels_denoise")) == 6 and len(_kernels("kernels_denoise_tiles")) == 7
    assert not any("robust" in k or "trim" in k for k in list(_kernels("kernels_denoise")) + list(_kernels("kernels_denoise_tiles")))


def test_the_trim_unit_is_built_like_the_robust_resolve():
    """The trim count is bit for bit rene_resolve_robust's: the unit that computes it takes that unit's flags, the prepare the denoiser's."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"\$\(HIPCC\) \$\(ROBUSTFLAGS\) \$\(RESFLAGS\) -c -o \$@ kernels_denoise_trim\.hip", mk)
    assert re.search(r"\$\(HIPCC\) \$\(HIPFLAGS\) \$\(RESFLAGS\) -c -o \$@ kernels_denoise_robust\.hip", mk)
