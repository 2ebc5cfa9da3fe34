#!/usr/bin/env python3
"""tools/summarize_denoise_profiles.py DIR TAG -- reduce the passes tools/denoise_prof.sh left in DIR (prof_dn_<size>_<pass>.json, written by
tools/extract_pass.py) to profiles/<TAG>_denoise_<size>.txt: the kernel-trace totals, and per dispatch of the LAST rene_denoise call of the
run its duration under the counter pass, wave-level VALU instructions, and the bytes the L2 exchanged with the fabric.

VALU issue fraction = SQ_INSTS_VALU x 64 lanes / duration / 78.64 Tlane-op/s (bench.py's peak: 1024 SIMDs, one wave64 VALU instruction per two
cycles at 2.4 GHz).  FETCH_SIZE is doubled (gfx950 tallies a 128-byte request as 64 bytes); Infinity-Cache hits are counted in both sizes, so
they say what crossed the L2's memory side, not what came from HBM."""
import json
import os
import sys

d, tag = sys.argv[1], sys.argv[2]
PEAK_LANE_OPS, PEAK_BW = 78.6432e12, 6.3e12
for size in ("1920x1080", "7680x4320"):
    w, h = map(int, size.split("x"))
    px = w * h
    load = lambda p: json.load(open(os.path.join(d, f"prof_dn_{size}_{p}.json")))
    lines = [f"# rene_denoise on cornell_box({w}, {h}) at 8 spp, defaults (five iterations; steps 1, 2, 4 staged in LDS): tools/denoise_prof.sh",
             f"# {px} pixels; one pass per counter group, --pmc never combined with --stats",
             "## rocprofv3 --kernel-trace --stats: kernel, calls, total us, average us (three rene_denoise calls: a warm-up and two)"]
    for name, calls, total, avg, _ in load("stats")["top_kernels"]:
        if "denoise" in name or "atrous" in name:
            lines.append(f"{name.split('(')[0].replace('void rene::', ''):32s} calls={calls:3d} total_us={total:10.1f} avg_us={avg:9.1f}")
    per = {}
    for p in ("sq1", "fetch", "write"):
        for name, disp, counter, value, dur, vgpr, sgpr, lds, grid in load(p)["dispatches"]:
            if "denoise" in name or "atrous" in name:
                e = per.setdefault(disp, {"name": name.split("(")[0].replace("void rene::", ""), "lds": lds, "vgpr": vgpr})
                e[counter] = value
                e.setdefault("dur_" + p, dur)
    ids = sorted(per)[-7:]  # the last call: prepare, five passes, finalize
    lines.append("## per dispatch of the last call, in launch order (durations in us are those of the pass that took the counter)")
    tot = {"us": 0.0, "valu": 0.0, "rd": 0.0, "wr": 0.0}
    for i in ids:
        e = per[i]
        us = e["dur_sq1"] * 1e-3
        valu = e["SQ_INSTS_VALU"]
        rd, wr = 2 * e["FETCH_SIZE"] * 1024, e["WRITE_SIZE"] * 1024
        for k, v in (("us", us), ("valu", valu), ("rd", rd), ("wr", wr)):
            tot[k] += v
        lines.append(f"{e['name']:26s} lds={e['lds']:6d} vgpr={e['vgpr']:3d} us={us:8.1f} (fetch pass {e['dur_fetch'] * 1e-3:8.1f}) valu_wave_insts={valu:12.0f} "
                     f"lane_ops_per_pixel={valu * 64 / px:7.1f} trans_f32_per_pixel={e['SQ_INSTS_VALU_TRANS_F32'] * 64 / px:5.1f} valu_issue_frac={valu * 64 / (us * 1e-6) / PEAK_LANE_OPS:5.3f} "
                     f"lds_insts_per_pixel={e['SQ_INSTS_LDS'] * 64 / px:5.1f} vmem_rd_per_pixel={e['SQ_INSTS_VMEM_RD'] * 64 / px:5.1f} "
                     f"read_MB={rd / 1e6:8.1f} write_MB={wr / 1e6:8.1f} bytes_per_s={(rd + wr) / (us * 1e-6) / 1e12:5.2f}e12 ({(rd + wr) / (us * 1e-6) / PEAK_BW:4.2f} of 6.3e12)")
    lines.append(f"total                      us={tot['us']:8.1f} lane_ops_per_pixel={tot['valu'] * 64 / px:7.1f} valu_issue_frac={tot['valu'] * 64 / (tot['us'] * 1e-6) / PEAK_LANE_OPS:5.3f} "
                 f"read_MB={tot['rd'] / 1e6:8.1f} write_MB={tot['wr'] / 1e6:8.1f} bytes_per_s={(tot['rd'] + tot['wr']) / (tot['us'] * 1e-6) / 1e12:5.2f}e12")
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", f"{tag}_denoise_{size}.txt")
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
