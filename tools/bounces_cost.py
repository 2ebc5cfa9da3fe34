"""tools/bounces_cost.py [OUT.json]: what the bounce pass costs beside the direct-light pass and beside a render of the same frames (DESIGN.md
section 4c).

cornell_box at 1024 x 1024 (the item loop, the Matte instantiation) and dragon_class at 1920 x 1080 (a BVH of 870 000 triangles), 16 frames, in ONE
process.  On one context per scene, whose stream is a torch stream, rene_bounces and rene_direct, each into a tensor of the caller's, and
rene_render of the same frames (behind a rene_reset outside the window) take turns: 21 rounds after three warm-up rounds, a different call first in
every round; each call sits between two HIP events on that stream and is waited for.  The passes' windows hold what the calls enqueue -- the
seeds' upload, the memset of the records, the kernel.  Medians and 10th - 90th percentiles, in ms, and the ratios of the medians; beside them what
the pass found: the mean path length, the longest path, and how far its total lies from the render's image.  Default output:
profiles/bounces_cost.json."""
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
        bounces = torch.empty(api.bounces_bytes(W, H), dtype=torch.uint8, device="cuda:0")
        direct = torch.empty(api.direct_bytes(W, H), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

        calls = (("rene_bounces", lambda: r.bounces_into(bounces, 0, FRAMES)), ("rene_direct", lambda: r.direct_into(direct, 0, FRAMES)),
                 ("rene_render", lambda: r.render(0, FRAMES)))
        times = {what: [] for what, _ in calls}
        for k in range(WARM + REPS):
            for j in range(len(calls)):
                what, call = calls[(j + k) % len(calls)]
                if what == "rene_render":
                    r.reset()
                    r.sync()
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record(stream)
                call()
                stop.record(stream)
                stop.synchronize()
                r.sync()
                if k >= WARM:
                    times[what].append(start.elapsed_time(stop))
        rec = np.frombuffer(bounces.cpu().numpy().tobytes(), api.abi.BOUNCES_DTYPE).reshape(H, W)
        beauty = r.download(0)[..., :3]  # (the last call of the last round that rendered left frames 0 .. 15 there)
        total = api.bounces_sum(rec)
        off = (np.abs(total - beauty) > 1e-2 * (1 + np.abs(beauty))).any(axis=-1)
        out = {k: figures(v) for k, v in times.items()}
        out["bounces / render (medians)"] = round(out["rene_bounces"]["median"] / out["rene_render"]["median"], 4)
        out["bounces / direct (medians)"] = round(out["rene_bounces"]["median"] / out["rene_direct"]["median"], 4)
        out["mean path length"] = round(float(api.bounces_mean_length(rec).mean()), 4)
        out["longest path"] = int(rec["length_max"].max())
        out["share of pixels whose total is off the render's by more than 1e-2 (1 + beauty)"] = round(float(off.mean()), 6)
        print(name, json.dumps(out), flush=True)
    return out


def main():
    import torch
    from rene_amd import scenes
    if not torch.cuda.is_available():
        sys.exit("tools/bounces_cost.py measures on a GPU and there is none")
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bounces_cost.json")
    cases = (("cornell_box 1024 1024", scenes.cornell_box(1024, 1024)), ("dragon_class 1920 1080", scenes.dragon_class()))
    results = {f"{name} {FRAMES}": measure(name, scene) for name, scene in cases}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"unit": "ms", "what": "HIP events on the context's stream around rene_bounces and rene_direct (caller's tensors) and rene_render of the same 16 frames, taking turns, one process",
                   "reps": REPS, "warm": WARM, "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
