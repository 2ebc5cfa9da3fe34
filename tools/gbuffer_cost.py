"""tools/gbuffer_cost.py [OUT.json]: what the geometry pass costs beside the render of the same frames.

cornell_box (the item loop) and dragon_class (a BVH of 870 000 triangles), both at 1920 x 1080, in ONE process.  On one context per scene, whose
stream is a torch stream, rene_gbuffer of 16 frames into a tensor of the caller's and rene_render of 16 frames alternate, 21 times each after three
warm-up rounds, a different one first in every other round; each call sits between two HIP events on that stream and is waited for.  The pass's
window holds what the call enqueues -- the seeds' upload, the memset of the records, the kernel; the render's holds its launch.  Medians and
10th - 90th percentiles, in ms, and the ratio of the medians.  Default output: profiles/gbuffer_cost.json."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARM, FRAMES = 21, 3, 16
W, H = 1920, 1080


def figures(values):
    v = np.asarray(values, np.float64)
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4), "n": int(v.size)}


def measure(name, scene):
    import torch
    from rene_amd import api
    stream = torch.cuda.Stream()
    times = {"rene_gbuffer": [], "rene_render": []}
    with api.Renderer(scene, stream_ptr=stream.cuda_stream) as r:
        dst = torch.empty(api.gbuffer_bytes(W, H), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        done = [0]

        def gbuffer():
            r.gbuffer_into(dst, 0, FRAMES)

        def render():
            r.render(done[0], FRAMES)
            done[0] += FRAMES

        calls = (("rene_gbuffer", gbuffer), ("rene_render", render))
        for k in range(WARM + REPS):
            for j in range(2):
                what, call = calls[(j + k) % 2]
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record(stream)
                call()
                stop.record(stream)
                stop.synchronize()
                r.sync()
                if k >= WARM:
                    times[what].append(start.elapsed_time(stop))
        rec = np.frombuffer(dst.cpu().numpy().tobytes(), api.abi.GBUFFER_DTYPE)
        coverage = float((rec["hits"].astype(np.float64) / FRAMES).mean())
    out = {k: figures(v) for k, v in times.items()}
    out["gbuffer / render (medians)"] = round(out["rene_gbuffer"]["median"] / out["rene_render"]["median"], 4)
    out["mean coverage"] = round(coverage, 4)
    print(name, json.dumps(out), flush=True)
    return out


def main():
    import torch
    from rene_amd import scenes
    if not torch.cuda.is_available():
        sys.exit("tools/gbuffer_cost.py measures on a GPU and there is none")
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gbuffer_cost.json")
    results = {f"{name} {W} {H} {FRAMES}": measure(name, build(W, H)) for name, build in (("cornell_box", scenes.cornell_box), ("dragon_class", scenes.dragon_class))}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"unit": "ms", "what": "HIP events on the context's stream around rene_gbuffer (16 frames, caller's tensor) and rene_render (16 frames), alternating, one process",
                   "reps": REPS, "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
