"""tools/occlusion_cost.py [OUT.json]: what the occlusion pass costs beside the geometry pass over the same frames.

cornell_box at 1024 x 1024 (the item loop) and dragon_class at 1920 x 1080 (a BVH of 870 000 triangles), in ONE process.  On one context per scene,
whose stream is a torch stream, and for every setting -- 1 and 4 rays per sample, a radius of 1e5 and one of about a hundredth of the scene's
extent -- rene_occlusion and rene_gbuffer of the same 16 frames, each into a tensor of the caller's, alternate: 41 pairs after five warm-up pairs,
a different one first in every other pair; each call sits between two HIP events on that stream and is waited for.  Either window holds what the
call enqueues -- the seeds' upload, the memset of the records, the kernel.  Medians and 10th - 90th percentiles, in ms, the ratio of the medians
and beside it 1 + rays, the queries a hitting sample makes.  Default output: profiles/occlusion_cost.json."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARM, FRAMES = 41, 5, 16
RAYS = (1, 4)
FAR = 1e5


def figures(values):
    v = np.asarray(values, np.float64)
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4), "n": int(v.size)}


def measure(name, scene, near):
    import torch
    from rene_amd import api
    stream = torch.cuda.Stream()
    W, H = scene.film.xresolution, scene.film.yresolution
    results = {}
    with api.Renderer(scene, stream_ptr=stream.cuda_stream) as r:
        occ = torch.empty(api.occlusion_bytes(W, H), dtype=torch.uint8, device="cuda:0")
        geo = torch.empty(api.gbuffer_bytes(W, H), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        for rays in RAYS:
            for radius in (FAR, near):
                times = {"rene_occlusion": [], "rene_gbuffer": []}
                calls = (("rene_occlusion", lambda: r.occlusion_into(occ, 0, FRAMES, rays, radius)), ("rene_gbuffer", lambda: r.gbuffer_into(geo, 0, FRAMES)))
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
                rec = np.frombuffer(occ.cpu().numpy().tobytes(), api.abi.OCCLUSION_DTYPE)
                out = {k: figures(v) for k, v in times.items()}
                out["occlusion / gbuffer (medians)"] = round(out["rene_occlusion"]["median"] / out["rene_gbuffer"]["median"], 4)
                out["queries per hitting sample"] = 1 + rays
                out["mean coverage"] = round(float(rec["hits"].sum() / (FRAMES * rec.size)), 4)
                out["mean occlusion"] = round(float(rec["occluded"].sum() / max(int(rec["rays"].sum()), 1)), 4)
                print(name, rays, radius, json.dumps(out), flush=True)
                results[f"rays {rays} radius {radius:g}"] = out
    return results


def main():
    import torch
    from rene_amd import scenes
    if not torch.cuda.is_available():
        sys.exit("tools/occlusion_cost.py measures on a GPU and there is none")
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "occlusion_cost.json")
    # (the Cornell box is 2 units wide and high; dragon_class is that room around a displaced sphere)
    cases = (("cornell_box 1024 1024", scenes.cornell_box(1024, 1024), 0.02), ("dragon_class 1920 1080", scenes.dragon_class(), 0.02))
    results = {f"{name} {FRAMES}": measure(name, scene, near) for name, scene, near in cases}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"unit": "ms", "what": "HIP events on the context's stream around rene_occlusion and rene_gbuffer (16 frames each, caller's tensors), alternating, one process",
                   "reps": REPS, "warm": WARM, "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
