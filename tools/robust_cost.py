"""What the firefly-robust resolve costs: times robust_tiles_kernel against noise_tiles_kernel -- which reads the same
128 bytes per pixel slot and writes nothing per pixel -- on the same context at 1920x1080 @ 16 and 7680x4320 @ 8, by the HIP events both calls
take under RENE_DEBUG: five warm-up calls, then 41 alternating pairs, medians.  `python tools/robust_cost.py [OUT_DIR]` on an MI355X; writes
robust_cost.json and the raw log."""
import json, os, re, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rene_amd import api, scenes

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "prof_out")
os.makedirs(OUT, exist_ok=True)
log = os.path.join(OUT, "robust_cost_stderr.txt")
fd = os.open(log, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
saved = os.dup(2)
result = {}
for (w, h), spp in (((1920, 1080), 16), ((7680, 4320), 8)):
    with api.Renderer(scenes.cornell_box(w, h)) as r:
        r.render(0, spp)
        r.sync()
        for _ in range(5):  # warm-up: code objects, buffers
            r.estimate_noise()
            r.resolve_robust()
        os.dup2(fd, 2)
        os.write(2, f"== {w} x {h}\n".encode())
        os.environ["RENE_DEBUG"] = "1"
        for _ in range(41):
            r.estimate_noise()
            r.resolve_robust()
        del os.environ["RENE_DEBUG"]
        os.dup2(saved, 2)
        s = r.resolve_robust()
    text = open(log).read().split(f"== {w} x {h}\n")[1]
    noise = [float(x) for x in re.findall(r"noise estimate .* ms: kernel ([0-9.]+)", text)]
    robust = [float(x) for x in re.findall(r"robust resolve .* ms: kernel ([0-9.]+)", text)]
    q = lambda v: dict(n=len(v), median=statistics.median(v), min=min(v), max=max(v), p10=sorted(v)[len(v) // 10], p90=sorted(v)[len(v) * 9 // 10])
    tiles = ((w + 31) // 32) * ((h + 31) // 32)
    bytes_read, bytes_written = tiles * 1024 * 8 * 16, w * h * 16
    result[f"{w}x{h}"] = dict(robust_tiles_kernel_ms=q(robust), noise_tiles_kernel_ms=q(noise), ratio_of_medians=statistics.median(robust) / statistics.median(noise),
                              byte_ratio=(bytes_read + bytes_written) / bytes_read, spp=spp, tiles=tiles, chain_bytes_layer0=bytes_read, image_bytes=bytes_written,
                              robust_GBps_at_median=(bytes_read + bytes_written) / statistics.median(robust) / 1e6,
                              noise_GBps_at_median=bytes_read / statistics.median(noise) / 1e6, kept_energy=s.kept_energy,
                              trimmed_share=s.n_trimmed / s.n_pixels)
    print(w, h, json.dumps(result[f"{w}x{h}"]), flush=True)
json.dump(result, open(os.path.join(OUT, "robust_cost.json"), "w"), indent=1)
