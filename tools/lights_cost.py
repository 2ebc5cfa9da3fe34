"""tools/lights_cost.py [OUT.json]: what the light-group pass costs beside the bounce pass of the same build over the same frames (DESIGN.md section
4c): the same path loop, plus the adds into the lane's LDS column and the fold of the column when a sample ends.

cornell_box at 1024 x 1024 (the item loop, the Matte instantiation) and dragon_class at 1920 x 1080 (a BVH of 870 000 triangles), 16 frames, in ONE
process.  On one context per scene, whose stream is a torch stream, rene_lights (the library's grouping) and rene_bounces, each into a tensor of the
caller's, take turns: 21 rounds after three warm-up rounds, the other call first in every other round; each call sits between two HIP events on
that stream and is waited for.  The windows hold what the calls enqueue -- the seeds' (and the tables') upload, the memset of the records, the
kernel.  Medians and 10th - 90th percentiles, in ms, and the ratio of the medians; beside them the groups in use, the share of lit samples and how
far the groups' total lies from the bounce pass's.  Default output: profiles/lights_cost.json."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARM, FRAMES = 21, 3, 16


def figures(values):
    v = np.asarray(values, np.float64)
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4), "n": int(v.size)}


def measure(name, scene):
    import torch
    from rene_amd import api
    stream = torch.cuda.Stream()
    W, H = scene.film.xresolution, scene.film.yresolution
    with api.Renderer(scene, stream_ptr=stream.cuda_stream) as r:
        lights = torch.empty(api.lights_bytes(W, H), dtype=torch.uint8, device="cuda:0")
        bounces = torch.empty(api.bounces_bytes(W, H), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        _, used = r.light_groups()

        calls = (("rene_lights", lambda: r.lights_into(lights, 0, FRAMES)), ("rene_bounces", lambda: r.bounces_into(bounces, 0, FRAMES)))
        times = {what: [] for what, _ in calls}
        for k in range(WARM + REPS):
            for j in range(len(calls)):
                what, call = calls[(j + k) % len(calls)]
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record(stream)
                call()
                stop.record(stream)
                stop.synchronize()
                r.sync()
                if k >= WARM:
                    times[what].append(start.elapsed_time(stop))
        rec = np.frombuffer(lights.cpu().numpy().tobytes(), api.abi.LIGHTS_DTYPE).reshape(H, W)
        brec = np.frombuffer(bounces.cpu().numpy().tobytes(), api.abi.BOUNCES_DTYPE).reshape(H, W)
        a, b = api.lights_sum(rec).astype(np.float64), api.bounces_sum(brec).astype(np.float64)
        M = FRAMES * 50 * (2 + len(scene.lights))
        off = (np.abs(a - b) > 4 * M * 2.0 ** -24 * np.maximum(a, b)).any(axis=-1)
        out = {k: figures(v) for k, v in times.items()}
        out["lights / bounces (medians)"] = round(out["rene_lights"]["median"] / out["rene_bounces"]["median"], 4)
        out["groups in use"] = int(used)
        out["share of lit samples"] = round(float(rec["lit"].sum(dtype=np.uint64)) / float(rec["n"].sum(dtype=np.uint64)), 4)
        out["share of pixels whose total is off the bounce pass's by more than 4 M 2^-24 max"] = round(float(off.mean()), 6)
        print(name, json.dumps(out), flush=True)
    return out


def main():
    import torch
    from rene_amd import scenes
    if not torch.cuda.is_available():
        sys.exit("tools/lights_cost.py measures on a GPU and there is none")
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lights_cost.json")
    cases = (("cornell_box 1024 1024", scenes.cornell_box(1024, 1024)), ("dragon_class 1920 1080", scenes.dragon_class()))
    results = {f"{name} {FRAMES}": measure(name, scene) for name, scene in cases}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"unit": "ms", "what": "HIP events on the context's stream around rene_lights and rene_bounces (caller's tensors) over the same 16 frames, taking turns, one process",
                   "reps": REPS, "warm": WARM, "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
