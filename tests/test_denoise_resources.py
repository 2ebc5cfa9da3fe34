"""CPU: what the compiler reports for the denoiser's gfx950 kernels (rene_amd/csrc/kernels_denoise.res and kernels_denoise_trim.res, written by the
Makefile with `-Rpass-analysis=kernel-resource-usage`): exactly the catalogue of instantiations, no scratch, no spills, the LDS-staged passes
small enough for two workgroups per compute unit, and the streaming kernels with registers to spare."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "rene_amd", "csrc")
LDS_PER_CU = 160 * 1024
PASS_STEPS = (0, 1, 2, 4)  # the direct pass and the three staged ones


def _kernels(unit):
    text = open(os.path.join(CSRC, unit + ".res")).read()
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", text, re.S):
        g = lambda key: int(re.search(re.escape(key) + r": (\d+)", m.group(2)).group(1))
        out[m.group(1)] = {"sgpr": g("TotalSGPRs"), "vgpr": g("VGPRs"), "scratch": g("ScratchSize [bytes/lane]"),
                           "occupancy": g("Occupancy [waves/SIMD]"), "sgpr_spill": g("SGPRs Spill"), "vgpr_spill": g("VGPRs Spill"),
                           "lds": int(m.group(3))}
    return out


def _b(*flags):
    return "I" + "".join(f"Lb{int(f)}E" for f in flags)  # the mangled bool template arguments


def _one(ks, name, args=""):
    """The kernel `name` (its instantiation `args`) of ks: the mangled name is <length><name>, then I<args>...E for a template."""
    hit = [k for k in ks if f"{len(name)}{name}{args or 'E'}" in k]
    assert len(hit) == 1, (name, args, sorted(ks))
    return hit[0]


# denoise_prepare_kernel<TILES, PACKED, TRIM>
PREPARES = {"plain": (0, 0, 0), "tiles": (1, 0, 0), "packed tiles": (1, 1, 0), "trimmed": (0, 0, 1), "trimmed tiles": (1, 0, 1)}


def _catalogue():
    ks, trim = _kernels("kernels_denoise"), _kernels("kernels_denoise_trim")
    cat = {"prepare " + what: _one(ks, "denoise_prepare_kernel", _b(*flags)) for what, flags in PREPARES.items()}
    for masked in (False, True):
        for s in PASS_STEPS:
            cat[f"pass {s} {masked}"] = _one(ks, "atrous_pass_kernel", f"ILi{s}E" + _b(masked)[1:])
        cat[f"finalize {masked}"] = _one(ks, "denoise_finalize_kernel", _b(masked))
    cat["mean"] = _one(ks, "denoise_mean_kernel")
    cat["place"] = _one(ks, "denoise_shard_place_kernel")
    return ks, trim, cat


def test_the_units_hold_exactly_the_catalogue_without_scratch_or_spills(hip_lib):
    ks, trim, cat = _catalogue()
    assert len(cat) == 17 and len(set(cat.values())) == 17 and set(cat.values()) == set(ks), sorted(ks)  # 5 prepare, 8 pass, 2 finalize, mean, place
    assert len(trim) == 1 and _one(trim, "denoise_trim_kernel")
    for name, k in {**ks, **trim}.items():
        assert k["scratch"] == 0 and k["sgpr_spill"] == 0 and k["vgpr_spill"] == 0, (name, k)


def _staged_passes_leave_room_for_two_workgroups_per_cu(masked):
    ks, _, cat = _catalogue()
    for s in PASS_STEPS:
        k = ks[cat[f"pass {s} {masked}"]]
        if s == 0:
            assert k["lds"] == 0, (masked, k)
            continue
        assert 0 < k["lds"] <= 80 * 1024 and 2 * k["lds"] <= LDS_PER_CU, (s, masked, k)
        assert k["occupancy"] >= 2, (s, masked, k)  # a workgroup is four waves, one per SIMD: two workgroups per CU = two waves per SIMD
        assert k["lds"] == (32 + 4 * s) * (8 + 4 * s) * 48, (s, masked, k)  # 32 x 8 tile + halo of 2 s, three 16-byte records per pixel


def test_staged_passes_leave_room_for_two_workgroups_per_cu(hip_lib):
    _staged_passes_leave_room_for_two_workgroups_per_cu(False)


def test_staged_masked_passes_leave_room_for_two_workgroups_per_cu(hip_lib):
    _staged_passes_leave_room_for_two_workgroups_per_cu(True)  # the mask travels in the records: the layout is the unmasked passes'


def test_streaming_kernels_are_not_limited_by_registers(hip_lib):
    ks, trim, cat = _catalogue()
    for what in ("prepare packed tiles", "place"):  # the tile-shard kernels
        k = ks[cat[what]]
        assert k["lds"] == 0 and k["occupancy"] >= 4, (what, k)
    trimmed = {what: ks[cat[what]] for what in ("prepare trimmed", "prepare trimmed tiles")}
    trimmed["trim"] = next(iter(trim.values()))
    for what, k in trimmed.items():  # eight float4 records in flight and room for every wave a SIMD can hold
        assert k["lds"] == 0 and k["vgpr"] <= 64 and k["occupancy"] >= 8, (what, k)


def test_the_trim_unit_is_built_like_the_robust_resolve():
    """The trim count is bit for bit rene_resolve_robust's: the unit that computes it takes that unit's flags, the prepare the denoiser's."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"\$\(HIPCC\) \$\(ROBUSTFLAGS\) \$\(RESFLAGS\) -c -o \$@ kernels_denoise_trim\.hip", mk)
    assert re.search(r"\$\(HIPCC\) \$\(HIPFLAGS\) \$\(RESFLAGS\) -c -o \$@ kernels_denoise\.hip", mk)
