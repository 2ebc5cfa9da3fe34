"""What adaptive sampling costs and saves, on one MI355X:

  mask     what a switched-off tile costs: Cornell 1024^2, one 64-frame launch with every tile active against the same launch with three tiles
           in four switched off (its items still pass through the version protocol, empty), alternating, medians -- against the ideal of a
           quarter of the full launch;
  job      what an adaptive job saves: a uniform job rendered until worst_tile_noise <= T (the schedule of render_until on the worst tile)
           against render_adaptive(T) with dilate 0 and 1, on Cornell 1024^2 and dragon-class 1920x1080; T = the uniform job's worst-tile
           figure at 256 frames; paths, wall-clock job time (estimates and mask changes included) and the final worst tile of each.

`python tools/adaptive_cost.py [OUT_DIR] [mask|job ...]`; writes adaptive_cost.json."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from rene_amd import api, scenes

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "prof_out")
WHAT = sys.argv[2:] or ["mask", "job"]
os.makedirs(OUT, exist_ok=True)
result = {}


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


if "mask" in WHAT:
    s = scenes.cornell_box(1024, 1024)
    ty = tx = 32
    quarter = np.zeros((ty, tx), np.uint8)
    quarter[::2, ::2] = 1  # one tile in four goes on, spread over the image

    def launch(r, mask):
        r.reset()
        if mask is not None:
            r.set_active_tiles(mask)
        r.sync()
        def go():
            r.render(0, 64)
            r.sync()
        return timed(go), r.stats().last_launch_ms

    with api.Renderer(s) as r:
        for _ in range(3):
            launch(r, None), launch(r, quarter)
        full, part = [], []
        for _ in range(15):
            full.append(launch(r, None))
            part.append(launch(r, quarter))
        paths_full = 64 * 1024 * 1024
    med = lambda v, i: statistics.median(x[i] for x in v)
    f_ms, p_ms = med(full, 1), med(part, 1)
    inactive_px = 1024 * 1024 * 3 // 4
    result["mask"] = dict(scene="cornell 1024x1024, one launch of 64 frames", runs=len(full), full_kernel_ms=f_ms, quarter_kernel_ms=p_ms, ideal_quarter_ms=f_ms / 4,
                          full_wall_ms=med(full, 0), quarter_wall_ms=med(part, 0), full_kernel_min_max=[min(x[1] for x in full), max(x[1] for x in full)],
                          quarter_kernel_min_max=[min(x[1] for x in part), max(x[1] for x in part)],
                          ns_per_inactive_pixel=(p_ms - f_ms / 4) * 1e6 / inactive_px, ns_per_active_pixel_frame=f_ms * 1e6 / paths_full)
    print("mask", json.dumps(result["mask"]), flush=True)


def uniform_until(r, target, cap, batch):
    """render_until's schedule with the worst tile as the figure."""
    done = min(batch, cap)
    r.render(0, done)
    est = r.estimate_noise()
    while est.worst_tile_noise > target and done < cap:
        need = int(min(np.ceil(done * (est.worst_tile_noise / target) ** 2), 0xFFFFFFFF))
        n = api.next_batch(done, need, batch, cap)
        r.render(done, n)
        done += n
        est = r.estimate_noise()
    return done, est


if "job" in WHAT:
    result["job"] = {}
    for name, make in (("cornell 1024x1024", lambda: scenes.cornell_box(1024, 1024)), ("dragon-class 1920x1080", lambda: scenes.dragon_class(1920, 1080))):
        s = make()
        cap, batch = 4096, 64
        with api.Renderer(s) as r:
            r.render(0, 256)
            target = r.estimate_noise().worst_tile_noise
            rows = {}
            for label, run in (("uniform", lambda: uniform_until(r, target, cap, batch)),
                               ("adaptive dilate 0", lambda: r.render_adaptive(target, cap, batch, 0)),
                               ("adaptive dilate 1", lambda: r.render_adaptive(target, cap, batch, 1))):
                ms = []
                for rep in range(3):
                    r.reset()
                    r.sync()
                    t0 = time.perf_counter()
                    got, est = run()
                    r.sync()
                    ms.append((time.perf_counter() - t0) * 1e3)
                st = r.stats().as_dict()
                frames = r.tile_frames()
                rows[label] = dict(job_ms=statistics.median(ms), job_ms_all=ms, paths=st["paths"], kernel_ms=st["kernel_ms"], launches=st["launches"],
                                   frames_max=int(frames.max()), frames_min=int(frames.min()), frames_mean=float(frames.mean()),
                                   worst_tile_noise=est.worst_tile_noise, noise=est.noise)
                print(name, label, json.dumps(rows[label]), flush=True)
            result["job"][name] = dict(target=target, cap=cap, batch=batch, **rows)

json.dump(result, open(os.path.join(OUT, "adaptive_cost.json"), "w"), indent=1)
