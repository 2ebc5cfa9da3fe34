"""What the feature export costs: times features_kernel against robust_tiles_kernel -- which reads the same 128 bytes of
chain records per pixel slot and writes 16 bytes per pixel -- on the same context at 1920x1080 @ 16 and 7680x4320 @ 8, by the HIP events both
calls take under RENE_DEBUG: five warm-up calls, then 41 alternating pairs per configuration, medians and the 10th .. 90th percentiles.
Configurations: the default mask (COLOR | ALBEDO | NORMAL) fp32 [H][W][C], and all seven features fp16 [C][H][W].  The expectation is the robust
kernel's time multiplied by the ratio of the bytes moved.  `python tools/features_cost.py [OUT_DIR [extra configuration ...]]` on an MI355X; writes
features_cost.json and the raw log."""
import json, os, re, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rene_amd import abi, api, scenes

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "prof_out")
os.makedirs(OUT, exist_ok=True)
log = os.path.join(OUT, "features_cost_stderr.txt")
fd = os.open(log, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
saved = os.dup(2)
CONFIGS = {"default_f32_hwc": (abi.FEATURE_DEFAULT, abi.FEATURES_F32, abi.FEATURES_HWC), "all_f16_chw": (abi.FEATURE_ALL, abi.FEATURES_F16, abi.FEATURES_CHW)}
# further names after OUT_DIR add the other corners, to tell a layout's or an element size's share of a shortfall
EXTRA = {"all_f32_chw": (abi.FEATURE_ALL, abi.FEATURES_F32, abi.FEATURES_CHW), "all_f16_hwc": (abi.FEATURE_ALL, abi.FEATURES_F16, abi.FEATURES_HWC),
         "all_f32_hwc": (abi.FEATURE_ALL, abi.FEATURES_F32, abi.FEATURES_HWC), "default_f16_chw": (abi.FEATURE_DEFAULT, abi.FEATURES_F16, abi.FEATURES_CHW)}
CONFIGS.update({n: EXTRA[n] for n in sys.argv[2:]})
q = lambda v: dict(n=len(v), median=statistics.median(v), min=min(v), max=max(v), p10=sorted(v)[len(v) // 10], p90=sorted(v)[len(v) * 9 // 10])
result = {}
for (w, h), spp in (((1920, 1080), 16), ((7680, 4320), 8)):
    with api.Renderer(scenes.cornell_box(w, h)) as r:
        r.render(0, spp)
        r.sync()
        tiles = ((w + 31) // 32) * ((h + 31) // 32)
        chain_bytes, robust_bytes = tiles * 1024 * 8 * 16, tiles * 1024 * 8 * 16 + w * h * 16
        for name, (mask, fmt, layout) in CONFIGS.items():
            p = api.feature_params_default()
            p.features, p.format, p.layout = mask, fmt, layout
            export = lambda: api._check(api.lib().rene_export_features(r._h, p, None, 0))
            for _ in range(5):  # warm-up: code objects, buffers
                r.resolve_robust()
                export()
            os.dup2(fd, 2)
            os.write(2, f"== {w} x {h} {name}\n".encode())
            os.environ["RENE_DEBUG"] = "1"
            for _ in range(41):
                r.resolve_robust()
                export()
            del os.environ["RENE_DEBUG"]
            os.dup2(saved, 2)
            text = open(log).read().split(f"== {w} x {h} {name}\n")[1]
            robust = [float(x) for x in re.findall(r"robust resolve .* ms: kernel ([0-9.]+)", text)]
            feat = [float(x) for x in re.findall(r"feature export .* ms: kernel ([0-9.]+)", text)]
            channels = api.feature_channels(mask)
            guides = sum(1 for b in (abi.FEATURE_ALBEDO, abi.FEATURE_NORMAL) if mask & b)
            read = (chain_bytes if mask & (abi.FEATURE_COLOR | abi.FEATURE_VARIANCE | abi.FEATURE_HALF_A | abi.FEATURE_HALF_B) else 0) + guides * w * h * 16
            written = channels * w * h * (2 if fmt == abi.FEATURES_F16 else 4)
            ratio, byte_ratio = statistics.median(feat) / statistics.median(robust), (read + written) / robust_bytes
            result[f"{w}x{h} {name}"] = dict(features_kernel_ms=q(feat), robust_tiles_kernel_ms=q(robust), ratio_of_medians=ratio, byte_ratio=byte_ratio,
                                             ratio_over_byte_ratio=ratio / byte_ratio, spp=spp, tiles=tiles, channels=channels, bytes_read=read, bytes_written=written,
                                             robust_bytes=robust_bytes, features_GBps_at_median=(read + written) / statistics.median(feat) / 1e6,
                                             robust_GBps_at_median=robust_bytes / statistics.median(robust) / 1e6)
            print(w, h, name, json.dumps(result[f"{w}x{h} {name}"]), flush=True)
json.dump(result, open(os.path.join(OUT, "features_cost.json"), "w"), indent=1)
