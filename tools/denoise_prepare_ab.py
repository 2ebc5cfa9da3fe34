"""tools/denoise_prepare_ab.py OUT.json [YARDSTICK.so THIS.so]: the denoiser's five prepare kernels, and the calls they belong to, of two builds of the
library in rene_amd/csrc/ (default: librene_hip_parent.so, built from the parent commit and copied there by hand, against librene_hip.so),
alternating the two libraries child process by child process within one session (RENE_HIP_LIB).  cornell_box at 1920 x 1080 @ 16 frames and
7680 x 4320 @ 8; the times are the library's own HIP events between its launches (RENE_DEBUG=1 prints them per kernel).  Per round the median of
21 calls; a kernel is within the yardstick's spread if the median of its round medians lies between the yardstick's lowest and highest round."""
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS, REPS = 5, 21
SIZES = ((1920, 1080, 16), (7680, 4320, 8))
CALLS = ("plain", "trimmed", "tiles", "trimmed tiles", "packed")


def child():
    from rene_amd import api, scenes
    for w, h, spp in SIZES:
        with api.Renderer(scenes.cornell_box(w, h)) as r:
            r.render(0, spp)
            calls = {"plain": r.denoise, "trimmed": lambda: r.denoise(robust=True), "tiles": r.denoise_tiles, "trimmed tiles": lambda: r.denoise_tiles(robust=True),
                     "packed": r.denoise_shard_prepare}
            for name in CALLS:
                print(f"[ab] warm-up {name}", file=sys.stderr, flush=True)
                calls[name]()
            for _ in range(REPS):
                for name in CALLS:
                    print(f"[ab] {w}x{h} {name}", file=sys.stderr, flush=True)
                    calls[name]()


def run(lib):
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, RENE_DEBUG="1", RENE_HIP_LIB=lib),
                       stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        print(f"child with {lib} ended with {p.returncode}: stopping", flush=True)
        sys.exit(1)
    out, key = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("[ab] "):
            key = None if "warm-up" in line else line[5:]
            continue
        if key is None:
            continue
        m = re.search(r"ms: (?:packed )?prepare (\S+?),? ", line + " ")
        if m:
            out.setdefault(key + " prepare", []).append(float(m.group(1)))
        m = re.search(r"; total (\S+)", line)
        if m:
            out.setdefault(key + " call total", []).append(float(m.group(1)))
    return {k: float(np.median(v)) for k, v in out.items()}


def main():
    yard, this = sys.argv[2:4] if len(sys.argv) > 3 else ("librene_hip_parent.so", "librene_hip.so")
    rounds = {yard: [], this: []}
    for k in range(ROUNDS):
        for lib in rounds:
            rounds[lib].append(run(lib))
            print(f"round {k} {lib} done", flush=True)
    result = {}
    for key in rounds[this][0]:
        a = [r[key] for r in rounds[yard]]
        b = [r[key] for r in rounds[this]]
        result[key] = {"parent round medians": a, "this round medians": b, "parent median": float(np.median(a)), "parent min": min(a), "parent max": max(a),
                       "this median": float(np.median(b)), "within parent spread": bool(min(a) <= float(np.median(b)) <= max(a))}
        print(f"{key:40s} parent {np.median(a):.4f} [{min(a):.4f} .. {max(a):.4f}]  this {np.median(b):.4f} [{min(b):.4f} .. {max(b):.4f}]", flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump({"unit": "ms, HIP events between the library's launches; medians of %d calls per round, %d alternating rounds" % (REPS, ROUNDS), "results": result}, f, indent=1)


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
