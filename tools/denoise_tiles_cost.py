"""tools/denoise_tiles_cost.py [OUT.json]: what rene_denoise_tiles costs beside rene_denoise.

On ONE even context the two calls alternate, 41 times each, at 1920 x 1080 @ 16 frames and at 7680 x 4320 @ 8 frames (cornell_box): the yardstick is
the existing call in the same session.  Then one adaptive context at 1920 x 1080 (a checkerboard of 16- and 32-frame tiles, one tile in eight never
rendered), rene_denoise_tiles alone.  The times are the library's own HIP events between its launches (RENE_DEBUG=1 prints them per kernel): the
measuring runs in a child process started with that variable, whose log this process reads.  Medians and 10th - 90th percentiles, in ms."""
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 41
SIZES = ((1920, 1080, 16), (7680, 4320, 8))


def child():
    from rene_amd import api, scenes
    for w, h, spp in SIZES:
        with api.Renderer(scenes.cornell_box(w, h)) as r:
            r.render(0, spp)
            print("[cost] warm-up", file=sys.stderr, flush=True)
            r.denoise()  # allocation, code objects
            r.denoise_tiles()
            print(f"[cost] even {w} {h} {spp}", file=sys.stderr, flush=True)
            for _ in range(REPS):
                r.denoise()
                r.denoise_tiles()
    w, h = SIZES[0][:2]
    with api.Renderer(scenes.cornell_box(w, h)) as r:
        ty, tx = (h + 31) // 32, (w + 31) // 32
        y, x = np.mgrid[0:ty, 0:tx]
        never = (x + 3 * y) % 8 == 0
        r.set_active_tiles(~never)
        r.render(0, 16)
        r.set_active_tiles(~never & ((x + y) % 2 == 0))
        r.render(16, 16)
        print("[cost] warm-up", file=sys.stderr, flush=True)
        r.denoise_tiles()
        print(f"[cost] adaptive {w} {h} 16/32", file=sys.stderr, flush=True)
        for _ in range(REPS):
            r.denoise_tiles()


def figures(values):
    v = np.asarray(values, np.float64)
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4), "n": int(v.size)}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "denoise_tiles_cost.json")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, RENE_DEBUG="1"), stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        sys.exit(p.returncode)
    result, section = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("[cost] "):
            section = line[len("[cost] "):]
            result[section] = {}
            continue
        m = re.match(r"\[rene\] denoise(, tile by tile,)? .*ms: (.*); total (\S+)", line)
        if not m or section is None:
            continue
        call = result[section].setdefault("rene_denoise_tiles" if m.group(1) else "rene_denoise", {})
        call.setdefault("total", []).append(float(m.group(3)))
        for part in m.group(2).split(", "):
            name, ms = part.rsplit(" ", 1)
            call.setdefault(name, []).append(float(ms))
    result.pop("warm-up", None)
    for section, calls in result.items():
        for call, parts in calls.items():
            calls[call] = {k: figures(v) for k, v in parts.items()}
            t = calls[call]["total"]
            print(f"{section:28s} {call:20s} total median {t['median']:.4f} ms (p10 {t['p10']:.4f}, p90 {t['p90']:.4f}, n {t['n']})")
            print("    " + ", ".join(f"{k} {v['median']:.4f}" for k, v in calls[call].items() if k != "total"))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"unit": "ms, HIP events between the library's launches", "reps": REPS, "results": result}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
