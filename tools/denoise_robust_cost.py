"""tools/denoise_robust_cost.py [OUT.json]: what the trimmed prepare of rene_denoise_robust costs beside rene_denoise's prepare.

On ONE context the two calls alternate, 41 times each, at 1920 x 1080 @ 16 frames and at 7680 x 4320 @ 8 frames (cornell_box): the yardstick is the
existing call in the same session.  The times are the library's own HIP events between its launches (RENE_DEBUG=1 prints them per kernel -- the
robust call's trim kernel on a line of its own): the measuring runs in a child process started with that variable, whose log this process reads.
Medians and 10th - 90th percentiles, in ms; `ratio` = (trim + prepare of the robust call) / (prepare of the plain call), of the medians."""
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
            r.denoise(robust=True)
            print(f"[cost] {w} {h} {spp}", file=sys.stderr, flush=True)
            for _ in range(REPS):
                r.denoise()
                r.denoise(robust=True)


def figures(values):
    v = np.asarray(values, np.float64)
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4), "n": int(v.size)}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "denoise_robust_cost.json")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, RENE_DEBUG="1"), stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        sys.exit(p.returncode)
    result, section, trim = {}, None, None
    for line in p.stderr.splitlines():
        if line.startswith("[cost] "):
            section = line[len("[cost] "):]
            result[section] = {}
            continue
        m = re.match(r"\[rene\] denoise, trimmed prepare .*ms: trim (\S+)", line)
        if m:
            trim = float(m.group(1))  # the robust call's first line; its second is a plain call's
            continue
        m = re.match(r"\[rene\] denoise .*ms: (.*); total (\S+)", line)
        if not m or section is None:
            continue
        call = result[section].setdefault("rene_denoise_robust" if trim is not None else "rene_denoise", {})
        for part in m.group(1).split(", "):
            name, ms = part.rsplit(" ", 1)
            call.setdefault(name, []).append(float(ms))
        if trim is not None:
            call.setdefault("trim", []).append(trim)
            call.setdefault("trim + prepare", []).append(trim + call["prepare"][-1])
        call.setdefault("total", []).append(float(m.group(2)) + (trim or 0.0))
        trim = None
    result.pop("warm-up", None)
    for section, calls in result.items():
        for call, parts in calls.items():
            calls[call] = {k: figures(v) for k, v in parts.items()}
        ratio = calls["rene_denoise_robust"]["trim + prepare"]["median"] / calls["rene_denoise"]["prepare"]["median"]
        calls["ratio"] = round(ratio, 3)
        print(f"{section}: prepare {calls['rene_denoise']['prepare']}, robust trim {calls['rene_denoise_robust']['trim']}, robust prepare "
              f"{calls['rene_denoise_robust']['prepare']}; (trim + prepare) / prepare = {ratio:.3f}; totals {calls['rene_denoise']['total']['median']:.4f} and "
              f"{calls['rene_denoise_robust']['total']['median']:.4f} ms")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"unit": "ms, HIP events between the library's launches", "reps": REPS, "results": result}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
