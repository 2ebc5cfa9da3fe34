"""What the noise estimate costs: times noise_tiles_kernel against denoise_prepare_kernel -- which reads the same
chains and more -- on the same context at 1920x1080 and 7680x4320, by the HIP events both calls take under RENE_DEBUG: five warm-up
calls, then 41 alternating pairs, medians.  `python tools/noise_cost.py [OUT_DIR]` on an MI355X; writes noise_cost.json and the raw log."""
import json, os, re, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rene_amd import api, scenes

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "prof_out")
os.makedirs(OUT, exist_ok=True)
log = os.path.join(OUT, "noise_cost_stderr.txt")
fd = os.open(log, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
saved = os.dup(2)
result = {}
for (w, h), spp in (((1920, 1080), 16), ((7680, 4320), 8)):
    with api.Renderer(scenes.cornell_box(w, h)) as r:
        r.render(0, spp)
        r.sync()
        for _ in range(5):  # warm-up: code objects, buffers
            r.estimate_noise()
            r.denoise(iterations=1)
        os.dup2(fd, 2)
        os.write(2, f"== {w} x {h}\n".encode())
        os.environ["RENE_DEBUG"] = "1"
        for _ in range(41):
            r.estimate_noise()
            r.denoise(iterations=1)
        del os.environ["RENE_DEBUG"]
        os.dup2(saved, 2)
        est = r.estimate_noise()
    text = open(log).read().split(f"== {w} x {h}\n")[1]
    noise = [float(x) for x in re.findall(r"noise estimate .* ms: kernel ([0-9.]+)", text)]
    prep = [float(x) for x in re.findall(r"denoise .* ms: prepare ([0-9.]+)", text)]
    q = lambda v: dict(n=len(v), median=statistics.median(v), min=min(v), max=max(v), p10=sorted(v)[len(v) // 10], p90=sorted(v)[len(v) * 9 // 10])
    tiles = ((w + 31) // 32) * ((h + 31) // 32)
    bytes_read = tiles * 1024 * 8 * 16
    result[f"{w}x{h}"] = dict(noise_tiles_kernel_ms=q(noise), denoise_prepare_kernel_ms=q(prep), spp=spp, tiles=tiles, chain_bytes_layer0=bytes_read,
                              noise_GBps_at_median=bytes_read / statistics.median(noise) / 1e6, noise=est.noise, rel_rmse=est.rel_rmse)
    print(w, h, json.dumps(result[f"{w}x{h}"]), flush=True)
json.dump(result, open(os.path.join(OUT, "noise_cost.json"), "w"), indent=1)
