"""tools/denoise_shard_cost.py [OUT.json]: what the denoiser's tile-shard kernels cost.

cornell_box, 1920 x 1080 @ 8 frames.  On ONE unsharded context rene_denoise_tiles and rene_denoise_shard_prepare alternate, 41 times each: the
yardstick of the packed prepare is the masked prepare of rene_denoise_tiles in the same session -- both read the same chains and write the same
bytes.  Between them shard 0 of 2 of the same job is placed on that context: the place kernel's time for one rank of two.  The times are the
library's own HIP events around its launches (RENE_DEBUG=1 prints them per kernel): the measuring runs in a child process started with that
variable, whose log this process reads.  Medians and 10th - 90th percentiles, in ms."""
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 41
W, H, SPP = 1920, 1080, 8


def child():
    from rene_amd import abi, api, scenes
    with api.Renderer(scenes.cornell_box(W, H)) as r, api.Renderer(scenes.cornell_box(W, H), shard_mode=abi.SHARD_TILES, shard_rank=0, shard_count=2) as s:
        r.render(0, SPP)
        s.render(0, SPP)
        s.denoise_shard_prepare()
        half = s.denoise_shard_buffer()
        print("[cost] warm-up", file=sys.stderr, flush=True)
        for _ in range(5):  # allocations, code objects
            r.denoise_tiles()
            r.denoise_shard_prepare()
            r.denoise_place_shard(half)
        print(f"[cost] {W} {H} {SPP}", file=sys.stderr, flush=True)
        for _ in range(REPS):
            r.denoise_tiles()
            r.denoise_shard_prepare()
            r.denoise_place_shard(half)


def figures(values):
    v = np.asarray(values, np.float64)
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4), "n": int(v.size)}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "denoise_shard_cost.json")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, RENE_DEBUG="1"), stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        sys.exit(p.returncode)
    patterns = {"masked prepare (rene_denoise_tiles)": r"\[rene\] denoise, tile by tile, .*ms: prepare (\S+),",
                "packed prepare (rene_denoise_shard_prepare, shard 0 of 1)": r"\[rene\] denoise shard 0 of 1, .*ms: packed prepare (\S+)",
                "place (rene_denoise_place_shard, shard 0 of 2)": r"\[rene\] denoise shard 0 of 2 placed, .*ms: place (\S+)"}
    result, section = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("[cost] "):
            section = line[len("[cost] "):]
            result[section] = {}
            continue
        for name, pattern in patterns.items():
            m = re.match(pattern, line)
            if m and section is not None:
                result[section].setdefault(name, []).append(float(m.group(1)))
    result.pop("warm-up", None)
    for section, kernels in result.items():
        for name, values in kernels.items():
            kernels[name] = f = figures(values)
            print(f"{section:16s} {name:60s} median {f['median']:.4f} ms (p10 {f['p10']:.4f}, p90 {f['p90']:.4f}, n {f['n']})")
        a, b = kernels.get("packed prepare (rene_denoise_shard_prepare, shard 0 of 1)"), kernels.get("masked prepare (rene_denoise_tiles)")
        if a and b:
            print(f"{section:16s} packed / masked prepare: {a['median'] / b['median']:.3f}")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"unit": "ms, HIP events around the library's launches", "reps": REPS, "results": result}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
